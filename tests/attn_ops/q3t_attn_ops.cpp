// q3t_attn_ops.cpp — test-only C entry points over the decode / prefill attention launchers attn_decode() and
// prefill_attn() (csrc/kernels.h), so that a test can run ONE launch on device buffers of its own and compare it with a
// reference of that operation (tests/test_gpu_attn_ops.py).  The vocoder's launchers have the same kind of shim in
// tests/ops/; this one is a library of its own so that the files the vocoder's tests load stay as they are.  Not part of
// the product: nothing here is exported through include/q3t_backend.h; the library links libq3t.so and calls the
// q3t:: launchers on the null stream, then synchronises.  Every entry returns 0, or -1 with the error text in err.
#include <cstdint>
#include <cstring>
#include <string>

#include "kernels.h"

using namespace q3t;

extern "C" {

// AttnParams / PrefillAttnParams (csrc/kernels.h) field by field, pointers as device addresses (0: null); dbg stays null
struct Q3tOpsAttn {
    uint64_t qkv, qn, kn, rope, pos, kc, vc, part, ticket, out, qkv_tab, tab_tok, tab_row0;
    float eps;
    int32_t n_ctx, S, nH, nKV, D, chunk, seqk, small, max_splits, tab_ld, tab_col;
};

struct Q3tOpsPrefillAttn {
    uint64_t qkv, qn, kn, rope, kc, vc, slot, out;
    float eps;
    int32_t n_ctx, n_utt, plen, nH, nKV, D, pad_;
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

}  // namespace

extern "C" {

int q3t_ops_attn_decode(const Q3tOpsAttn *d, char *err, int errlen) {
    AttnParams p;
    p.qkv = ptr<const float>(d->qkv); p.qn = ptr<const float>(d->qn); p.kn = ptr<const float>(d->kn); p.eps = d->eps;
    p.rope = ptr<const float>(d->rope); p.pos = ptr<const int>(d->pos);
    p.kc = ptr<uint16_t>(d->kc); p.vc = ptr<uint16_t>(d->vc);
    p.n_ctx = d->n_ctx; p.S = d->S; p.nH = d->nH; p.nKV = d->nKV; p.D = d->D;
    p.chunk = d->chunk; p.seqk = d->seqk; p.small = d->small; p.max_splits = d->max_splits;
    p.part = ptr<float>(d->part); p.ticket = ptr<unsigned>(d->ticket); p.out = ptr<uint16_t>(d->out);
    p.qkv_tab = ptr<const float>(d->qkv_tab); p.tab_tok = ptr<const int>(d->tab_tok);
    p.tab_ld = d->tab_ld; p.tab_col = d->tab_col; p.tab_row0 = (size_t)d->tab_row0;
    return finish(attn_decode(p, nullptr), err, errlen);
}

int q3t_ops_prefill_attn(const Q3tOpsPrefillAttn *d, char *err, int errlen) {
    PrefillAttnParams p;
    p.qkv = ptr<const float>(d->qkv); p.qn = ptr<const float>(d->qn); p.kn = ptr<const float>(d->kn); p.eps = d->eps;
    p.rope = ptr<const float>(d->rope); p.kc = ptr<uint16_t>(d->kc); p.vc = ptr<uint16_t>(d->vc);
    p.slot = ptr<const int>(d->slot);
    p.n_ctx = d->n_ctx; p.n_utt = d->n_utt; p.plen = d->plen; p.nH = d->nH; p.nKV = d->nKV; p.D = d->D;
    p.out = ptr<uint16_t>(d->out);
    return finish(prefill_attn(p, nullptr), err, errlen);
}

}  // extern "C"
