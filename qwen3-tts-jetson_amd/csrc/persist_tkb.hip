// persist_tkb.hip — the BATCHED talker decode step (2..64 slots, BASELINE configs[2]) as ONE persistent launch: the
// 28-layer stack, the final norm (hidden-state side output), the codec head and the CB0 selection of the next frame
// (src/tts_transformer.cpp:1376-1512 build_step_graph, :2416-2499 CB0 processing).  It replaces decoder_stack_mm's
// 7 launches per layer + head + select_tokens (engine.cpp) and computes the same bits: every projection is that
// graph's MFMA tile with the same K quarters, split-K slices and LDS sum order (persist_mm.h, gemm_mfma.hip), every
// residual + RMSNorm is k_resid_norm's arithmetic, the attention is k_attn_seq's source (attn_seq.h) and the selection
// is select_tokens' (select.h).
//
// Work per layer for S slots in NT token tiles of 32, one 256-thread workgroup per CU (persist_mm.h hand-offs):
//
//   job              count            workgroups        tile / input (per job)                      output
//   RN_A / RN_F      1 per slot       128 + 2b          x[b] += 4 slabs; RMSNorm -> f16 row          xnA / xnF [b]
//   QKV              64 x NT          [0, 64 NT)        64 rows x 32 tokens, K 1024                  qkv granules
//   ATT              8 per slot       u % 256, u = 8b+g (slot b, kv head g): the whole context          attn f16
//   O                16 x 4 x NT      [0, 64 NT)        64 rows x 32 tokens x K slice 512            slabO granules
//   GU               96 x NT          gj: [0, 128), odd slot wgs  32 SwiGLU units x 32 tokens           h f16
//   DN               16 x 4 x NT      [0, 64 NT)        64 rows x 32 tokens x K slice 768            slabD granules
//   HEAD             48 x NT          [0, 48 NT)        64 rows x 32 tokens, K 1024 (final xnA)      logits granules
//   SEL              1 per slot       128 + 2b          CB0 selection of the slot (+ logits row, commit)
//
// The residual stream of slot b never leaves its RN workgroup (4 values per thread for the whole step).  The attention
// units of a workgroup run in order u = w, w + 256: K/V chunk 0 of a unit is in flight before its QKV granules are
// polled.  Every wait is bounded (persist_dev.h SPIN_LIMIT): a protocol fault ends the launch with *err set and the
// engine falls back to the launch-per-op graph, which is bit-identical.
#include "persist.h"
#include "persist_mm.h"
#include "attn_seq.h"
#include "select.h"

#pragma clang fp contract(off)   // every rounding as written: bit-identical to k_gemm_mfma / k_resid_norm / k_attn_seq

namespace q3t {

namespace {
using namespace pmm;

constexpr int NL = 28, VPT = VOC / 256, NHP = VOC / 64;
constexpr StateLayout SL(VOC);
#ifndef TKB_NB
#define TKB_NB 4   // attention K/V ring depth (chunks of 32 KB per workgroup)
#endif

struct BLds {
    uint4 wl[4][32][64];   // the next job's A fragments / the K-quarter partials (persist_mm.h)
    SelLds sel;
    AttnSeqLds att;
    double dscr[4];
    PLayerW layers[NL];
};

// REC: the CB0 selection reads the slots' sampling records (p.sel.rec, per-utterance sampling); launched without it
// when p.sel.rec is null, so a call without records runs the code it ran before there were any
template <int NT, bool REC>
__global__ void __launch_bounds__(256, 1) k_tkb(const TkbParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    BLds &S = *reinterpret_cast<BLds *>(smem);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, w = blockIdx.x;
    Ctx X = make_ctx(p.state, SL, p.prof, p.S, S.wl);
    const Jobs J(w, NT, NHP, p.S);
    const int sw = w - SW0;
    const bool rn = J.slot && (sw & 1) == 0;   // slot b's residual row, norms and selection
    const int b = sw >> 1;
    const int nunits = NKV * p.S;
    for (int i = t; i < NL; i += 256) S.layers[i] = p.L[i];
    __syncthreads();

    // ---- the GEMM job sequence of this workgroup: every layer's four jobs, then the head (layer slot NL)
    auto W = weight_issue(
        S.wl, S.layers, NL, 1, NHP, J,
        [](WJob &j) {
            if (j.k == K_QKV) j.k = K_O;
            else if (j.k == K_O) j.k = K_GU;
            else if (j.k == K_GU) j.k = K_DN;
            else if (j.k == K_DN) {
                if (j.l + 1 < NL) { ++j.l; j.k = K_QKV; }
                else { j.l = NL; j.k = K_HEAD; }
            } else j.pass = 1;
        },
        [&](const WJob &) { return p.head; });
    W.issue();

    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);   // the RN workgroups' residual row (thread t: elements 4t .. 4t+3)

    for (int l = 0; l < NL; ++l) {
        const PLayerW &Lw = S.layers[l];
        // ---- RN_A: the layer's input row, normalised (layer 0: the step's input row)
        if (rn) {
            if (l == 0) x = ldf4(p.x_in + (size_t)b * H + 4 * t);
            else fold(X, x, b, SL.sld, X.tag(ph_of(l - 1, K_DN)));
            norm_pub(X, x, b, Lw.attn_norm, p.eps, S.dscr, SL.xna, K_RNA, X.tag(ph_of(l, K_RNA)), nullptr);
        }
        if (J.hq) {
            W.flush();
            job_qkv(X, SL, w, l);
            W.defer();   // the O weights after the attention units: their polls and K/V streams go first
        }
        // ---- ATT: units u = w, w + 256 (slot u / 8, kv head u % 8), the whole context of each, in turn as one chunk
        // stream (the second unit's first chunks in flight during the first unit's tail)
        if (w < nunits) {
            const uint32_t tq = X.tag(ph_of(l, K_QKV));
            const int nu = w + G < nunits ? 2 : 1, g = w & 7;
            const int ub[2] = {w >> 3, (w + G) >> 3};
            CPROF(ph_of(l, K_QKV), 0);
            attn_seq_stream<TKB_NB>(
                nu,
                [&](int k, int &pos, uint16_t *&kc, uint16_t *&vc, const float *&rope_row) {
                    pos = p.pos[ub[k]];
                    const size_t hoff = (size_t)l * p.kv_layer + ((size_t)ub[k] * NKV + g) * p.n_ctx * D;
                    kc = p.kc + hoff;
                    vc = p.vc + hoff;
                    rope_row = p.rope + (size_t)pos * D;
                },
                Lw.qn, Lw.kn, p.eps,
                [&](int k, int v, float (&xv)[2]) {   // wave v: q head 2g + v (v < 2), k (2), v (3) of slot ub[k]
                    const int row = v < 2 ? (2 * g + v) * D : v == 2 ? (NH + g) * D : (NH + NKV + g) * D;
                    u32x4_t gq[1];
                    poll_gran<1>(X, tq, gq, [&](u32x4_t (&r)[1]) {
                        const size_t o = SL.qkv + ((size_t)ub[k] * QKVN + row + lane) * 8;
                        const u32x2_t a = __builtin_amdgcn_raw_buffer_load_b64(X.rs, (int)o, 0, SC1V);
                        const u32x2_t c = __builtin_amdgcn_raw_buffer_load_b64(X.rs, (int)(o + 64 * 8), 0, SC1V);
                        r[0] = u32x4_t{a.x, a.y, c.x, c.y};
                    });
                    if (k == 0 && v == 0) CPROF(ph_of(l, K_QKV), 1);
                    xv[0] = __uint_as_float(gq[0].x);
                    xv[1] = __uint_as_float(gq[0].z);
                },
                [&](int k, int hd, int d, float y) {   // one half of the slot's attention row, fragment order
                    __builtin_amdgcn_raw_buffer_store_b16(f2h(y), X.rs, (int)SL.attn + fragoff(NH * D / 8, ub[k], (2 * g + hd) * D + d), 0, SC1);
                },
                [&](int k) {
                    if (k == 0) CPROF(ph_of(l, K_ATT), 3);
                    publish(X, K_ATT, w + k * G, X.tag(ph_of(l, K_ATT)));
                },
                S.att);
        }
        W.flush();
        if (J.hq) {
            // wave v multiplies head 4 z + v: the units of kv head 2 z + v / 2 of the tile's slots (its own wait, no barrier)
            job_o(X, SL, w, l, [&](int z, int tt, int nv, uint32_t tg) {
                wait_flags(X, K_ATT, nv, [&](int i) { return (32 * tt + i) * NKV + 2 * z + (wave >> 1); }, tg);
            });
            W.after_job();
        }
        // ---- RN_F
        if (rn) {
            fold(X, x, b, SL.slo, X.tag(ph_of(l, K_O)));
            norm_pub(X, x, b, Lw.ffn_norm, p.eps, S.dscr, SL.xnf, K_RNF, X.tag(ph_of(l, K_RNF)), nullptr);
        }
        if (J.hg) {
            W.flush();
            job_gu(X, SL, J.gj, l);
            W.after_job();
        }
        if (J.hq) {
            W.flush();
            job_dn(X, SL, w, l);
            W.after_job();
        }
    }
    // ---- final RMSNorm (output_norm, hidden-state side output) -> codec head -> CB0 selection
    if (rn) {
        fold(X, x, b, SL.sld, X.tag(ph_of(NL - 1, K_DN)));
        norm_pub(X, x, b, p.out_norm, p.eps, S.dscr, SL.xna, K_RNA, X.tag(ph_of(NL, K_RNA)), p.hidden);
    }
    if (J.hh) {
        W.flush();
        job_head(X, SL, w, NL, VOC, NHP);
    }
    if (rn) {
        CPROF(ph_of(NL, K_HEAD), 0);
        SelPre pre;   // the selection's per-slot inputs (done, frame, seed, seen bytes) before the poll, off the chain
        if (p.select) sel_prefetch<SEL_CB0, REC>(p.sel, b, pre);
        float v[SEL_VPT_MAX];
        poll_logits<VPT>(X, SL.lg, b, X.tag(ph_of(NL, K_HEAD)), v);
        CPROF(ph_of(NL, K_HEAD), 1);
        if (p.logits) {   // the logits row, as the per-op head GEMM writes it
            float *row = p.logits + (size_t)b * VOC + VPT * t;
#pragma unroll
            for (int k = 0; k < VPT / 4; ++k) *reinterpret_cast<float4 *>(row + 4 * k) = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
        }
        if (p.select) {
            const int tok = select_token_pre<SEL_CB0, REC>(p.sel, pre, v, S.sel);   // -1: slot done
            if (t == 0 && tok >= 0) select_commit(p.sel, b, tok);
        }
        CPROF(ph_of(NL, K_HEAD), 3);
    }
    exit_ticket(reinterpret_cast<unsigned *>(p.state + SL.ctr), X.seq);
}

constexpr size_t LDS = lds_bytes<BLds>();

}  // namespace

size_t tkb_state_bytes() { return SL.total; }
bool tkb_error(const uint8_t *state, hipStream_t s, bool *err) { return state_error(SL, state, s, err); }
bool tkb_clear(uint8_t *state, hipStream_t s) { return state_clear(SL, state, s); }
bool tkb_resident(int device) {
    return resident<&k_tkb<1, false>, &k_tkb<2, false>>(device, LDS) && resident<&k_tkb<1, true>, &k_tkb<2, true>>(device, LDS);
}

bool persist_talker_batched(const TkbParams &p, hipStream_t s) {
    if (!p.L || p.n_layers != NL || !p.head || !p.out_norm || !p.x_in || !p.hidden || !p.rope || !p.pos || !p.kc || !p.vc ||
        p.n_ctx < 1 || !p.state || p.S < 2 || p.S > SMAX || (p.select && (p.sel.mode != SEL_CB0 || p.sel.V != VOC || !p.sel.tokens))) {
        set_error("persist_talker_batched: bad parameters");
        return false;
    }
    if (p.select && p.sel.rec) return launch_by_tile_count<&k_tkb<1, true>, &k_tkb<2, true>>(p, LDS, s);
    return launch_by_tile_count<&k_tkb<1, false>, &k_tkb<2, false>>(p, LDS, s);
}

}  // namespace q3t
