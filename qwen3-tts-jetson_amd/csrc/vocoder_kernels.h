// vocoder_kernels.h — launchers of the vocoder (tokenizer decoder) kernels.
#pragma once
#include "q3t_common.h"

namespace q3t {

constexpr int CONV_MAX_TAPS = 7;

// SnakeBeta x + exp(-beta) sin^2(exp(alpha) x) with a = exp(alpha), ib = exp(-beta) (audio_tokenizer_decoder.cpp
// SnakeBeta).  The sine: reduce to [-0.5, 0.5] revolutions (v_rndne) and use the hardware v_sin_f32 -- ocml's sinf is
// ~30 VALU instructions with a range-reduction branch and ran twice per activation element of every residual unit;
// its result is rounded to f16 right after, so the ~1e-6 difference flips an f16 rounding only rarely.  Every kernel
// that applies SnakeBeta calls this one function, rounding each operation as written (no contraction), so a fused
// and an unfused launch sequence produce the same bits.
__device__ __forceinline__ float snake_apply(float z, float a, float ib) {
#pragma clang fp contract(off)
    const float r = (z * a) * 0.15915494309189535f;   // 1 / (2 pi)
    const float sn = __builtin_amdgcn_sinf(r - __builtin_rintf(r));
    return z + (sn * sn) * ib;
}
struct ConvTap { const uint16_t *w; int dj; };   // w: [C_out][C_in] f16 of one kernel tap; input row offset dj
// y[m*so + ob][co] = act(bias[co] + resid + sum_j sum_ci w_j[co][ci] * f16(snake(x[m + dj][ci])))
// x: [T_in][C_in] f32 (rows outside [0,T_in) read as 0 = causal zero padding); y: [T_out][C_out] f32
struct ConvParams {
    const float *x = nullptr;
    const uint16_t *xh = nullptr;   // alternative input: f16 rows [T_in][C_in] with SnakeBeta already applied (C_in % 8 == 0)
    int T_in = 0, C_in = 0;
    const float *snake_a = nullptr, *snake_ib = nullptr;   // exp(alpha), exp(-beta) per input channel (nullable)
    int n_taps = 0;
    ConvTap taps[CONV_MAX_TAPS];
    int dmin = 0, dmax = 0;
    float *y = nullptr;             // f32 output [T_out][ldy] (nullable when y16 is set)
    int C_out = 0, M = 0, so = 1, ob = 0;
    int ldy = 0;                    // row stride of y and resid (0: C_out)
    const float *bias = nullptr, *resid = nullptr;
    const float *scale = nullptr;   // per output channel, applied after the bias and before the residual
    int act = 0;   // 1 = tanh, 2 = ReLU, 3 = tanh(ReLU), 4 = GELU (ggml tanh form, f16 table); after the residual
    // optional f16 output of the same elements: y16[t][co] = f16(snake(v)) with exp(alpha) / exp(-beta) per output
    // channel (y16_a null: plain rounding) -- the NEXT conv's input, so no separate snake/round pass reads y back
    uint16_t *y16 = nullptr;
    const float *y16_a = nullptr, *y16_ib = nullptr;
    // transposed conv in one launch (multi-tile kernel): grid z = output phase phi of a stride-ct_st transposed conv
    // with ct_k taps [ct_k][C_out][C_in] at ct_w, trimmed by ct_trim; phase phi writes rows ct_st*m + phi < T_out
    // from taps k = (phi + trim) % st + j*st at input offset (phi + trim - k) / st.  taps/dmin/dmax/M/so/ob unused
    const uint16_t *ct_w = nullptr;
    int ct_k = 0, ct_st = 0, ct_trim = 0, T_out = 0;
    // utterance batch (grid z = nb x phases): nb independent sequences of the same length; utterance u's input rows
    // start xbs rows after u-1's (x / xh), its output rows (y, resid, y16) ybs rows after.  Causal padding stays
    // inside each utterance (rows outside [0, T_in) of its own segment read as 0)
    int nb = 1;
    int64_t xbs = 0, ybs = 0;
    int dev_skip = 0;   // development builds only (timing experiments): 1 weight loads, 2 window loads, 4 epilogue
    int xcd_tiles = 0;  // k_conv_mt 1-tap narrow variant: channel tiles of a row tile on one XCD (set by conv())
};
bool conv(const ConvParams &p, hipStream_t s);
// the kernel conv() launches for p (host arithmetic only: the tile count, the channel counts, the tap layout and the
// Q3T_CONV_* environment switches).  conv() launches by switching on this value, so the two cannot diverge.
enum { CONV_NONE = 0, CONV_GENERIC = 1, CONV_MT = 2, CONV_PD = 3 };
struct ConvKernel {
    int family = CONV_NONE;   // CONV_NONE: nothing is launched (empty or unsupported parameters)
    int RB = 0, NT = 0;       // k_conv_mt / k_conv_pd: 128 RB rows x NT output channels per workgroup
    int TW = 0;               // k_conv_mt: TW (taps staged per chunk); k_conv_pd: TAPS
    int MINB = 0;             // workgroups per CU of the launch bounds
    int xcd = 0;              // tiles taken in XCD order (ConvParams::xcd_tiles of the launch)
};
ConvKernel conv_kernel(const ConvParams &p);
// one 96-channel decoder residual unit as one launch (vocoder_resunit.hip), bit-identical to its two conv launches:
//   h = f16(snake2(conv7_dil(xh) + b1)) (kept on chip);  y = x + conv1(h) + b2;  y16 = f16(snake_next(y))
// xh / y16 are f16 [T][96] (different buffers: a tile's causal window reads rows of its neighbours), x / y f32 (may
// alias: in place; y null skips the f32 output); w1 [7][96][96], w2 [96][96] f16; nb utterances bs rows apart
struct ResUnitParams {
    const uint16_t *xh = nullptr;
    const float *x = nullptr;
    float *y = nullptr;
    uint16_t *y16 = nullptr;
    int T = 0, dil = 1;
    const uint16_t *w1 = nullptr, *w2 = nullptr;
    const float *b1 = nullptr, *a2 = nullptr, *ib2 = nullptr, *b2 = nullptr, *an = nullptr, *ibn = nullptr;
    int nb = 1;
    int64_t bs = 0;
};
bool resunit96(const ResUnitParams &p, hipStream_t s);
// out[t][c] = f16( snake(x[t][c]) ) (SnakeBeta x + exp(-beta) sin^2(exp(alpha) x), or plain rounding when a is null):
// the conv input computed ONCE per element instead of once per (output tile, tap window) inside k_conv
bool snake_f16(const float *x, const float *a, const float *ib, uint16_t *out, int64_t T, int C, hipStream_t s);
// out[t][:] = f16(norm(x[t][:])): mode 0 RMSNorm (x * scale) * w, mode 1 LayerNorm ((x - mean) * scale) * w + b;
// double sums as gemm_mfma's PRO_RMS / PRO_LN prologues (the input of a 1-tap conv used as a large-M GEMM)
bool norm_f16(const float *x, const float *w, const float *b, float eps, int mode, uint16_t *out, int T, int C,
              hipStream_t s);
// y[t] = tanh(bias + sum_j sum_ci w[j][ci] * xh[t + j - (K - 1)][ci]): the decoder's last conv (C_out = 1, K <= 8)
// nb utterances of T rows each, back to back (xh [nb][T][C], y [nb][T])
bool conv_out1(const uint16_t *xh, const uint16_t *w, const float *bias, float *y, int T, int C, int K, hipStream_t s,
               int nb = 1);
bool dwconv(const float *x, const uint16_t *w, const float *b, float *y, int T, int C, int K, hipStream_t s, int nb = 1);
// RoPE is applied to qkv's q and k columns in place; nb utterances of F frames each, causal within each
bool attn_prefill(float *qkv, const float *rope, uint16_t *out, int F, int nH, int D, hipStream_t s, int nb = 1);
// a vocoder stream's attention (Vocoder::stream_push): the n new frames at absolute positions P..P+n-1 against per-layer
// f32 caches kc / vc [max_frames][nH*D] of rotated keys and of values, rope [max_frames][D] indexed by position.
// voc_kv_append: attn_prefill's RoPE launch on the new rows -- q rotated in place in qkv [n][3*nH*D], rotated k and v
// written to cache rows P..P+n-1 (the caller guarantees P + n <= max_frames; rows before P are not touched).
// voc_attn_cached: out [n][nH*D] f16, bit-identical to rows P..P+n-1 of attn_prefill over the P + n frames; cache rows
// at or past P + n are never read.
bool voc_kv_append(float *qkv, const float *rope, float *kc, float *vc, int P, int n, int nH, int D, hipStream_t s);
bool voc_attn_cached(const float *qkv, const float *kc, const float *vc, uint16_t *out, int P, int n, int nH, int D,
                     hipStream_t s);
// The same for many streams in ONE launch each (Vocoder::stream_push_batch).  descs is a device array of n_streams
// descriptors; stream j's n new rows are rows row0 .. row0+n-1 of the packed qkv [sum n][3*nH*D] and out [sum n][nH*D],
// its caches of layer `layer` start layer * layer_stride floats into kc / vc.  Per stream the arithmetic is
// voc_kv_append's and voc_attn_cached's (one shared body each), so its bits do not depend on the batch around it.
// max_n / max_tiles: the largest n, and the largest tile count (P + n + 31) / 32 - P / 32, over the streams (the
// grids; a workgroup past its own stream's count returns at once).
struct VocStreamDesc {
    float *kc = nullptr, *vc = nullptr;   // [layers][max_frames][nH*D], layer 0
    const float *rope = nullptr;          // [max_frames][D]
    int64_t layer_stride = 0;             // max_frames * nH * D
    int32_t P = 0, n = 0, row0 = 0, pad_ = 0;
};
bool voc_kv_append_batch(float *qkv, const VocStreamDesc *descs, int n_streams, int max_n, int layer, int nH, int D,
                         hipStream_t s);
bool voc_attn_cached_batch(const float *qkv, uint16_t *out, const VocStreamDesc *descs, int n_streams, int max_tiles,
                           int layer, int nH, int D, hipStream_t s);
// n_descs independent copies of `n` floats each in one launch (descs: a device array; max_n: the largest n).  The
// carried state of a batched stream push: windows assembled from state and new rows, rows compacted, state written
// back.  Copies only.  A source and a destination of one launch must not overlap.  vec4: every n of the launch is a
// multiple of 4 and every pointer 16-byte aligned (16-byte moves).
struct VocCopyDesc {
    const float *src = nullptr;
    float *dst = nullptr;
    int64_t n = 0;
};
bool voc_copy_batch(const VocCopyDesc *descs, int n_descs, int64_t max_n, bool vec4, hipStream_t s);
bool codes_cols(const int32_t *codes, int *cols, int F, int ncb, hipStream_t s);

}  // namespace q3t
