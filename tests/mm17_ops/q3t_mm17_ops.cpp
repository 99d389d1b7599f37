// q3t_mm17_ops.cpp — test-only C entry points over the launchers that the 1.7B matrix-core path added shapes to:
// resid_norm() (rows up to 2,048 wide), select_embed_norm() (the H = 2,048 step embedding and the f32 projected-table
// source) and gemv() routed to the MFMA GEMM (csrc/kernels.h), so that a test can run ONE launch on device buffers of
// its own and compare it with a float64 numpy restatement (tests/test_gpu_mm17_ops.py).  A library of its own, like
// tests/queue_ops/, so that the files the other op tests load stay as they are.  Not part of the product: nothing here
// is exported through include/q3t_backend.h; the library links libq3t.so and calls the q3t:: launchers on the null
// stream, then synchronises.  Entries return >= 0, or -1 with the error text in err.
#include <cstdint>
#include <cstring>
#include <string>

#include "kernels.h"

using namespace q3t;

namespace {

template <typename T> T *ptr(uint64_t v) { return reinterpret_cast<T *>(static_cast<uintptr_t>(v)); }

int finish(bool ok, char *err, int errlen, int value = 0) {
    std::string msg;
    if (!ok) msg = last_error();
    else {
        const hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) return value;
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

// x [S][H] f32 (read and, with parts or xin, written), xin [S][H] or 0, parts [ksplit][S][H] or 0, nw [H], xn [S][H]
// f16, side [S][H] f32 or 0.  Returns the 1024-wide chunks per thread of the instantiation that ran (1: the narrow
// form every H <= 1,024 launches, 2: the wide form).
int q3t_m17_resid_norm(uint64_t xin, uint64_t x, uint64_t parts, int32_t ksplit, uint64_t nw, float eps, uint64_t xn,
                       uint64_t side, int32_t S, int32_t H, char *err, int errlen) {
    ResidNorm r;
    r.xin = ptr<const float>(xin); r.x = ptr<float>(x); r.parts = ptr<const float>(parts); r.ksplit = ksplit;
    r.nw = ptr<const float>(nw); r.eps = eps; r.xn = ptr<uint16_t>(xn); r.side = ptr<float>(side); r.S = S; r.H = H;
    return finish(resid_norm(r, nullptr), err, errlen, resid_norm_chunks(H));
}

// One code-predictor selection (SEL_CP, head `step`, greedy when temperature <= 0) over logits [S][V] fused with the
// next stage's input: nt = 1 with ftab != 0: the f32 row ftab[ftab_row0 + token] (token column tok_col0); nt = 1
// with tab0: the f16 row of tab0; nt = 16: the step embedding over tabs (device array of 16 tables) + tr / pad.
// tokens [S][16], codes [S][max_len][16], frame / done / tr_len [S], utt [S] u64, x [S][H] f32, xn [S][H] f16.
int q3t_m17_select_embed_norm(uint64_t logits, int32_t V, int32_t step, float temperature, uint64_t tokens, uint64_t codes,
                              int32_t max_len, uint64_t frame, uint64_t done, uint64_t utt, int32_t nt, int32_t tok_col0,
                              uint64_t tab0, uint64_t tabs, uint64_t tr, uint64_t tr_len, int32_t tr_ld, uint64_t pad,
                              uint64_t ftab, uint64_t ftab_row0, uint64_t x, uint64_t xn, uint64_t nw, float eps, int32_t H,
                              int32_t S, char *err, int errlen) {
    SelectSpec sp;
    sp.mode = SEL_CP; sp.V = V; sp.step = step; sp.temperature = temperature; sp.top_k = 50; sp.seed = 1;
    sp.tokens = ptr<int>(tokens); sp.codes = ptr<int32_t>(codes); sp.max_len = max_len; sp.ncb = 16;
    sp.frame = ptr<const int>(frame); sp.done = ptr<int>(done); sp.utt = ptr<const uint64_t>(utt);
    EmbedNorm en;
    en.nt = nt;
    en.gs.tok = ptr<const int>(tokens); en.gs.tok_ld = 16; en.gs.tok_col0 = tok_col0;
    en.gs.tab0 = ptr<const uint16_t>(tab0); en.gs.tabs = ptr<const uint16_t *const>(tabs);
    en.gs.tr = ptr<const float>(tr); en.gs.tr_len = ptr<const int>(tr_len); en.gs.frame = ptr<const int>(frame);
    en.gs.tr_ld = tr_ld; en.gs.pad = ptr<const float>(pad);
    en.ftab = ptr<const float>(ftab); en.ftab_row0 = (size_t)ftab_row0;
    en.x = ptr<float>(x); en.xn = ptr<uint16_t>(xn); en.nw = ptr<const float>(nw); en.eps = eps; en.H = H;
    return finish(select_embed_norm(sp, ptr<const float>(logits), en, S, nullptr), err, errlen);
}

// gemv() over f16 rows x [B][K]: W [N][K] f16; act 3 = SwiGLU (rows interleaved [gate16 | up16], out_f16 [B][N / 2]);
// parts != 0: split-K slabs [ksplit][B][N] f32; else out_f32 [B][N].  Returns 1 if the call was routed to the MFMA
// GEMM (gemm_mfma_supported), 0 if it ran on the vector kernel.
int q3t_m17_gemv(uint64_t W, int32_t N, int32_t K, int32_t B, uint64_t x, int32_t act, uint64_t out_f16, uint64_t out_f32,
                 int32_t ldo, uint64_t parts, int32_t ksplit, char *err, int errlen) {
    GemvParams g;
    g.W = ptr<const uint16_t>(W); g.N = N; g.K = K; g.B = B;
    g.pro = PRO_F16; g.x = ptr<const uint16_t>(x); g.ldx = K;
    g.act = act; g.out_f16 = ptr<uint16_t>(out_f16); g.out_f32 = ptr<float>(out_f32); g.ldo = ldo;
    g.parts = ptr<float>(parts); g.ksplit = parts ? ksplit : 1;
    const int routed = gemm_mfma_supported(g) ? 1 : 0;
    return finish(gemv(g, nullptr), err, errlen, routed);
}

}  // extern "C"
