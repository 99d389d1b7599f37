// q3t_ops.cpp — test-only C entry points over the vocoder's kernel launchers (csrc/vocoder_kernels.h), so that a test
// can run ONE operation on device buffers of its own and compare it with a reference of that operation.  Not part of
// the product: nothing here is exported through include/q3t_backend.h; the library links libq3t.so and calls the
// q3t:: launchers on the null stream, then synchronises.  Every entry returns 0, or -1 with the error text in err.
#include <cstdint>
#include <cstring>
#include <string>

#include "vocoder_kernels.h"

using namespace q3t;

extern "C" {

// A stride-1 conv as Vocoder::conv16 builds it: taps {w + j*C_out*C_in, j*dil - pad}; or, with ct_st != 0, a transposed
// conv in one launch as Vocoder::convT16 builds it (n_taps / dil / pad / M / so / ob unused).  Pointers are device
// addresses (0: null).
struct Q3tOpsConv {
    uint64_t x, xh, snake_a, snake_ib, w, y, y16, y16_a, y16_ib, bias, scale, resid, ct_w;
    int64_t xbs, ybs;
    int32_t T_in, C_in, C_out, M, n_taps, dil, pad, so, ob, ldy, act, nb;
    int32_t ct_k, ct_st, ct_trim, T_out;
};

struct Q3tOpsResUnit {
    uint64_t xh, x, y, y16, w1, w2, b1, a2, ib2, b2, an, ibn;
    int64_t bs;
    int32_t T, dil, nb, pad_;
};

}  // extern "C"

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

bool fill(const Q3tOpsConv &d, ConvParams &p, std::string &why) {
    p.x = ptr<const float>(d.x);
    p.xh = ptr<const uint16_t>(d.xh);
    p.T_in = d.T_in; p.C_in = d.C_in;
    p.snake_a = ptr<const float>(d.snake_a); p.snake_ib = ptr<const float>(d.snake_ib);
    p.y = ptr<float>(d.y); p.C_out = d.C_out; p.ldy = d.ldy;
    p.bias = ptr<const float>(d.bias); p.scale = ptr<const float>(d.scale); p.resid = ptr<const float>(d.resid);
    p.act = d.act;
    p.y16 = ptr<uint16_t>(d.y16); p.y16_a = ptr<const float>(d.y16_a); p.y16_ib = ptr<const float>(d.y16_ib);
    p.nb = d.nb; p.xbs = d.xbs; p.ybs = d.ybs;
    if (d.ct_st) {
        p.ct_w = ptr<const uint16_t>(d.ct_w); p.ct_k = d.ct_k; p.ct_st = d.ct_st; p.ct_trim = d.ct_trim; p.T_out = d.T_out;
        return true;
    }
    if (d.n_taps < 1 || d.n_taps > CONV_MAX_TAPS) { why = "q3t_ops: n_taps out of range"; return false; }
    p.n_taps = d.n_taps;
    const uint16_t *w = ptr<const uint16_t>(d.w);
    for (int j = 0; j < d.n_taps; ++j) p.taps[j] = ConvTap{w + (size_t)j * d.C_out * d.C_in, j * d.dil - d.pad};
    p.dmin = -d.pad; p.dmax = (d.n_taps - 1) * d.dil - d.pad;
    p.M = d.M; p.so = d.so; p.ob = d.ob;
    return true;
}

}  // namespace

extern "C" {

int q3t_ops_conv(const Q3tOpsConv *d, char *err, int errlen) {
    ConvParams p;
    std::string why;
    if (!fill(*d, p, why)) { set_error(why); return finish(false, err, errlen); }
    return finish(conv(p, nullptr), err, errlen);
}

// out[6] = family (0 none, 1 generic, 2 mt, 3 pd), RB, NT, TW or TAPS, MINB, xcd
int q3t_ops_conv_kernel(const Q3tOpsConv *d, int32_t *out) {
    ConvParams p;
    std::string why;
    ConvKernel k;
    if (fill(*d, p, why)) k = conv_kernel(p);
    out[0] = k.family; out[1] = k.RB; out[2] = k.NT; out[3] = k.TW; out[4] = k.MINB; out[5] = k.xcd;
    return 0;
}

int q3t_ops_resunit96(const Q3tOpsResUnit *d, char *err, int errlen) {
    ResUnitParams p;
    p.xh = ptr<const uint16_t>(d->xh); p.x = ptr<const float>(d->x); p.y = ptr<float>(d->y); p.y16 = ptr<uint16_t>(d->y16);
    p.T = d->T; p.dil = d->dil;
    p.w1 = ptr<const uint16_t>(d->w1); p.w2 = ptr<const uint16_t>(d->w2);
    p.b1 = ptr<const float>(d->b1); p.a2 = ptr<const float>(d->a2); p.ib2 = ptr<const float>(d->ib2);
    p.b2 = ptr<const float>(d->b2); p.an = ptr<const float>(d->an); p.ibn = ptr<const float>(d->ibn);
    p.nb = d->nb; p.bs = d->bs;
    return finish(resunit96(p, nullptr), err, errlen);
}

int q3t_ops_snake_f16(uint64_t x, uint64_t a, uint64_t ib, uint64_t out, int64_t T, int32_t C, char *err, int errlen) {
    return finish(snake_f16(ptr<const float>(x), ptr<const float>(a), ptr<const float>(ib), ptr<uint16_t>(out), T, C, nullptr),
                  err, errlen);
}

int q3t_ops_norm_f16(uint64_t x, uint64_t w, uint64_t b, float eps, int32_t mode, uint64_t out, int32_t T, int32_t C,
                     char *err, int errlen) {
    return finish(norm_f16(ptr<const float>(x), ptr<const float>(w), ptr<const float>(b), eps, mode, ptr<uint16_t>(out), T, C,
                           nullptr), err, errlen);
}

int q3t_ops_conv_out1(uint64_t xh, uint64_t w, uint64_t bias, uint64_t y, int32_t T, int32_t C, int32_t K, int32_t nb,
                      char *err, int errlen) {
    return finish(conv_out1(ptr<const uint16_t>(xh), ptr<const uint16_t>(w), ptr<const float>(bias), ptr<float>(y), T, C, K,
                            nullptr, nb), err, errlen);
}

int q3t_ops_dwconv(uint64_t x, uint64_t w, uint64_t b, uint64_t y, int32_t T, int32_t C, int32_t K, int32_t nb, char *err,
                   int errlen) {
    return finish(dwconv(ptr<const float>(x), ptr<const uint16_t>(w), ptr<const float>(b), ptr<float>(y), T, C, K, nullptr,
                         nb), err, errlen);
}

int q3t_ops_attn_prefill(uint64_t qkv, uint64_t rope, uint64_t out, int32_t F, int32_t nH, int32_t D, int32_t nb,
                         char *err, int errlen) {
    return finish(attn_prefill(ptr<float>(qkv), ptr<const float>(rope), ptr<uint16_t>(out), F, nH, D, nullptr, nb), err,
                  errlen);
}

}  // extern "C"
