// persist_cpb.hip — the BATCHED code-predictor frame (4..64 slots, BASELINE configs[2]) as ONE persistent launch:
// 16 passes of the 5-layer stack, lm_head[p-1] + token selection after pass p >= 1, and the next talker step's
// embedding (src/tts_transformer.cpp:2153-2340, src/trt_code_predictor.cpp:484-600,
// scripts/export_code_predictor.py:132-231).  It replaces the ~570-launch graph of decoder_stack_mm (engine.cpp) for one
// frame, and computes the same bits: every projection is that graph's MFMA tile with the same K quarters, the same
// split-K slices and the same LDS sum order (gemm_mfma.hip), every residual + RMSNorm is k_resid_norm's arithmetic, the
// attention is k_attn_small's source (attn_small.h) and the selection is k_select_embed_norm's (select.h).
//
// Work per layer for S slots in NT token tiles of 32 (NT = 1: S <= 32, NT = 2: S <= 64), one 256-thread workgroup per CU:
//
//   job              count            workgroups        tile / input (per job)                    output
//   RN_A / RN_F      1 per slot       128 + 2b          x[b] += 4 slabs; RMSNorm -> f16 row        xnA / xnF [b]
//   QKV              128 x NT         [0, 128 NT)       32 rows x 32 tokens, K 1024 (xnA 64 KB)    qkv f32
//   ATT              1 per slot       192 + b           8 kv groups (2 per wave), <= 16 positions  attn f16 [b]
//   O                32 x 4 x NT      [0, 128 NT)       32 rows x 32 tokens x K slice 512          slabO f32 [z]
//   GU               96 x NT          gj: [0, 128), odd slot wgs  64 rows (32 SwiGLU units) x 32 tokens  h f16
//   DN               32 x 4 x NT      [0, 128 NT)       32 rows x 32 tokens x K slice 768          slabD f32 [z]
//   HEAD (p >= 1)    64 x NT          [0, 64 NT)        32 rows x 32 tokens, K 1024 (final xnA)    logits f32
//   SEL  (p >= 1)    1 per slot       192 + b           top-k / argmax of the slot's row, commit; next pass's x[b]
//
// The residual stream of slot b never leaves its RN workgroup: x[b] lives in registers (4 values per thread) for the
// whole frame.  Hand-offs are MI355X_MICROARCH.md's flag form for bandwidth (hand-off table, row 1): every payload byte
// is stored with an agent-scope (sc1) store, each storing wave waits vmcnt(0), a workgroup barrier, then ONE lane
// stores the job's flag (sc1); a consumer wave polls the flags of exactly the producers whose bytes it reads (sc1
// loads) and then loads the payload with sc1 loads.  A flag carries ((seq << 10) + phase + 1): seq is bumped once per
// launch, so a flag of an earlier phase or launch never matches.  Payload buffers are single-buffered: every producer
// reaches its next write of a buffer only through a chain of jobs that needs every reader of the previous contents to
// have finished.  Every wait is bounded (persist_dev.h SPIN_LIMIT): a protocol fault ends the launch with *err set and
// the engine falls back to the launch-per-op graph, which is bit-identical.
#include "persist.h"
#include "persist_mm.h"
#include "attn_small.h"
#include "select.h"

#pragma clang fp contract(off)   // every rounding as written: bit-identical to k_gemm_mfma / k_resid_norm / k_attn_small

namespace q3t {

namespace {
using namespace pmm;

constexpr int NLC = 5, NPASS = 16, NHP = CPV / 64;
constexpr StateLayout SL(CPV);
__device__ __forceinline__ int ls_of(int pass, int l) { return pass * 6 + l; }   // layer slot (persist_mm.h ph_of); l = NLC: the head

struct BLds {
    // the next job's A fragments [wave][16 rt + 4c + j][lane] (LDS-DMA, issued one job ahead); once a job's MFMAs are
    // done, wave w's region holds its K-quarter partial tiles [rt][reg][lane] (f32)
    uint4 wl[4][32][64];
    SelLds sel;
    AttnSmallLds att[4];
    double dscr[4];
    int toks[16];
    PLayerW layers[NLC];
    const uint16_t *heads[16];
    const uint16_t *tabs[16];
};

// ---------------------------------------------------------------- the kernel
// REC: the selections read the slots' sampling records (p.sel.rec, per-utterance sampling); launched without it when
// p.sel.rec is null, so a call without records runs the code it ran before there were any
template <int NT, bool REC>
__global__ void __launch_bounds__(256, 1) k_cpb(const CpbParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    BLds &S = *reinterpret_cast<BLds *>(smem);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, w = blockIdx.x;
    Ctx X = make_ctx(p.state, SL, p.prof, p.S, S.wl);
    // GEMM jobs: 64 rows x one token tile; QKV / O / DN on [0, 64 NT), gate/up on [0, 96 NT), lm_head on [0, 32 NT)
    const Jobs J(w, NT, NHP, p.S);
    // slot workgroups: SW0 + 2b + hf for slot b, half hf (kv groups 4 hf .. 4 hf + 3); the even one (rn) also keeps the
    // slot's residual row, runs its norms and commits its selections
    const int sw = w - SW0;
    const bool slot = J.slot;
    const int b = sw >> 1, hf = sw & 1;
    const bool rn = slot && hf == 0;
    if (t < NLC) S.layers[t] = p.L[t];
    if (t < 15) S.heads[t] = p.heads[t];
    if (t < 16) S.tabs[t] = p.tabs[t];
    if (slot && t < 16) S.toks[t] = p.sel.tokens[b * 16 + t];
    __syncthreads();

    // ---- the GEMM job sequence of this workgroup: pass 0's last layer ends after QKV (only its K/V rows are ever read),
    // layer 0 of passes >= 1 has no QKV job (the per-token table)
    auto W = weight_issue(
        S.wl, S.layers, NLC, NPASS, NHP, J,
        [](WJob &j) {
            if (j.k == K_QKV) {
                if (j.pass == 0 && j.l == NLC - 1) { j.pass = 1; j.l = 0; }
                j.k = K_O;
            } else if (j.k == K_O) j.k = K_GU;
            else if (j.k == K_GU) j.k = K_DN;
            else if (j.k == K_DN) {
                if (j.l + 1 < NLC) { ++j.l; j.k = K_QKV; }
                else { j.l = NLC; j.k = K_HEAD; }
            } else { ++j.pass; j.l = 0; j.k = K_O; }
        },
        [&](const WJob &j) { return S.heads[j.pass - 1]; });
    W.issue();

    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);   // the RN workgroups' residual row (thread t: elements 4t .. 4t+3)

    for (int pass = 0; pass < NPASS; ++pass) {
        const int pos = slot ? p.pos[(size_t)pass * p.pos_ld + b] : 0;
        for (int l = 0; l < NLC; ++l) {
            const PLayerW &Lw = S.layers[l];
            const int ls = ls_of(pass, l);
            if (pass == 0 || l >= 1) {
                // ---- RN_A: the layer's input row, normalised (pass 0 layer 0: the talker hidden state)
                if (rn) {
                    if (pass == 0 && l == 0) x = ldf4(p.x_in + (size_t)b * H + 4 * t);
                    else fold(X, x, b, SL.sld, X.tag(ph_of(ls - 1, K_DN)));
                    norm_pub(X, x, b, Lw.attn_norm, p.eps, S.dscr, SL.xna, K_RNA, X.tag(ph_of(ls, K_RNA)), nullptr);
                }
                if (J.hq) {
                    W.flush();
                    job_qkv(X, SL, w, ls);
                    W.after_job();
                }
            }
            // ---- ATT: kv group 4 hf + wave of slot b (one wave each); its cached K / V rows are loaded before the wait
            if (slot) {
                const bool tab = pass >= 1 && l == 0;
                const int g = 4 * hf + wave;
                const size_t hoff = (size_t)l * p.kv_layer + (((size_t)b * NKV + g) * 16) * D;
                AttnSmallKV kv;
                attn_small_load_kv<true>(pos, p.kc + hoff, p.vc + hoff, kv);
                AttnSmallAux aux;
                attn_small_load_aux(p.rope + (size_t)pos * D, Lw.qn, Lw.kn, aux);
                float xs[4][2];
                if (tab) {   // layer 0 of passes 1..15: the per-token table row of the previous pass's token
                    attn_small_load_qkv<false>(p.qkvtab + ((size_t)(pass == 1 ? 0 : VOC + (pass - 2) * CPV) + S.toks[pass - 1]) * QKVN,
                                               g, NH, NKV, xs);
                } else {     // the QKV jobs' granules of slot b
                    const uint32_t tg = X.tag(ph_of(ls, K_QKV));
                    CPROF(ph_of(ls, K_QKV), 0);
                    u32x4_t gq[4];   // {v, e = 0} / {v, e = 1} of q0, q1, k, v (x, y: e 0; z, w: e 1)
                    poll_gran<4>(X, tg, gq, [&](u32x4_t (&r)[4]) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const size_t o = SL.qkv + ((size_t)b * QKVN + attn_small_src(g, v, NH, NKV) + lane) * 8;
                            const u32x2_t a = __builtin_amdgcn_raw_buffer_load_b64(X.rs, (int)o, 0, SC1V);
                            const u32x2_t c = __builtin_amdgcn_raw_buffer_load_b64(X.rs, (int)(o + 64 * 8), 0, SC1V);
                            r[v] = u32x4_t{a.x, a.y, c.x, c.y};
                        }
                    });
                    CPROF(ph_of(ls, K_QKV), 1);
#pragma unroll
                    for (int v = 0; v < 4; ++v) { xs[v][0] = __uint_as_float(gq[v].x); xs[v][1] = __uint_as_float(gq[v].z); }
                }
                uint16_t *const ab = reinterpret_cast<uint16_t *>(p.state + SL.attn);
                attn_small_compute<true>(kv, xs, aux, g, pos, p.eps, p.kc + hoff, p.vc + hoff,
                                         [&](int e) { return ab + fragoff(NH * D / 8, b, e) / 2; }, S.att[wave]
#ifdef CPB_ATT_STAMPS   // development: stamps inside the attention, phases (pass, 5, 1 + l), column k
                                         , [&](int k) { CPROF(pass * 48 + 41 + l, k); }
#endif
                );
                CPROF(ph_of(ls, K_ATT), 3);
                if (!(pass == 0 && l == NLC - 1)) publish(X, K_ATT, sw, X.tag(ph_of(ls, K_ATT)));
                else __syncthreads();
                W.flush();
            }
            if (pass == 0 && l == NLC - 1) continue;   // pass 0's last layer: only its K/V rows are ever read
            if (J.hq) {
                W.flush();
                // wave v multiplies heads 4 z + v: kv group (4 z + v) / 2, published by the slots' half (4 z + v) / 8 (wave 0
                // polls that half's flags of the tile's slots for the workgroup)
                job_o(X, SL, w, ls, [&](int z, int tt, int nv, uint32_t tg) {
                    wait_flags_wg(X, K_ATT, nv, [&](int i) { return 2 * (32 * tt + i) + ((4 * z) >> 3); }, tg);
                });
                W.after_job();
            }
            // ---- RN_F
            if (rn) {
                fold(X, x, b, SL.slo, X.tag(ph_of(ls, K_O)));
                norm_pub(X, x, b, Lw.ffn_norm, p.eps, S.dscr, SL.xnf, K_RNF, X.tag(ph_of(ls, K_RNF)), nullptr);
            }
            if (J.hg) {
                W.flush();
                job_gu(X, SL, J.gj, ls);
                W.after_job();
            }
            if (J.hq) {
                W.flush();
                job_dn(X, SL, w, ls);
                W.after_job();
            }
        }
        if (pass == 0) {   // pass 1's input: the codec_embd row of CB0 (k_gather_sum, one table)
            if (rn) {
                const uint2 u = *reinterpret_cast<const uint2 *>(S.tabs[0] + (size_t)S.toks[0] * H + 4 * t);
                x = make_float4(h2f(u.x & 0xffff), h2f(u.x >> 16), h2f(u.y & 0xffff), h2f(u.y >> 16));
            }
            continue;
        }
        // ---- final RMSNorm (output_norm) -> lm_head[pass - 1] -> selection of code `pass`
        const int lh = ls_of(pass, NLC);
        if (rn) {
            fold(X, x, b, SL.sld, X.tag(ph_of(lh - 1, K_DN)));
            norm_pub(X, x, b, p.out_norm, p.eps, S.dscr, SL.xna, K_RNA, X.tag(ph_of(lh, K_RNA)), nullptr);
        }
        if (J.hh) {
            W.flush();
            job_head(X, SL, w, lh, CPV, NHP);
            W.after_job();
        }
        if (slot) {   // both halves select (the same token); the even one commits it
            CPROF(ph_of(lh, K_HEAD), 0);
            SelectSpec sp = p.sel;
            sp.step = pass - 1;
            SelPre pre;   // the selection's per-slot inputs (done, frame, seed, utterance) before the poll, off the chain
            sel_prefetch<SEL_CP, REC>(sp, b, pre);
            float v[SEL_VPT_MAX];
            poll_logits<CPV / 256>(X, SL.lg, b, X.tag(ph_of(lh, K_HEAD)), v);
            CPROF(ph_of(lh, K_HEAD), 1);
            const int tok = select_token_pre<SEL_CP, REC>(sp, pre, v, S.sel);   // -1: slot done
            if (t == 0 && tok >= 0) {
                if (rn) select_commit(sp, b, tok);
                S.toks[pass] = tok;
            }
            __syncthreads();
            CPROF(ph_of(lh, K_HEAD), 3);
            if (!rn) {
            } else if (pass + 1 < NPASS) {   // the next pass's input: code_pred.codec_embd[pass - 1] row of this token
                const uint2 u = *reinterpret_cast<const uint2 *>(S.tabs[pass] + (size_t)S.toks[pass] * H + 4 * t);
                x = make_float4(h2f(u.x & 0xffff), h2f(u.x >> 16), h2f(u.y & 0xffff), h2f(u.y >> 16));
            } else {
                if (p.talker_next) {   // the next talker step's embedding + its layer-0 RMSNorm (k_select_embed_norm, nt 16)
                    float a[4];
                    {
                        const uint2 u = *reinterpret_cast<const uint2 *>(S.tabs[0] + (size_t)S.toks[0] * H + 4 * t);
                        a[0] = h2f(u.x & 0xffff); a[1] = h2f(u.x >> 16); a[2] = h2f(u.y & 0xffff); a[3] = h2f(u.y >> 16);
                    }
#pragma unroll
                    for (int j = 1; j < 16; ++j) {
                        const uint2 u = *reinterpret_cast<const uint2 *>(S.tabs[j] + (size_t)S.toks[j] * H + 4 * t);
                        a[0] += h2f(u.x & 0xffff); a[1] += h2f(u.x >> 16); a[2] += h2f(u.y & 0xffff); a[3] += h2f(u.y >> 16);
                    }
                    const int fr = p.frame[b];
                    const float *extra = fr < p.tr_len[b] ? p.tr + (size_t)b * p.tr_ld + (size_t)fr * H : p.pad + (size_t)b * H;
                    const float4 e = ldf4(extra + 4 * t);
                    a[0] += e.x; a[1] += e.y; a[2] += e.z; a[3] += e.w;
                    const float4 xt = make_float4(a[0], a[1], a[2], a[3]);
                    *reinterpret_cast<float4 *>(p.tx + (size_t)b * H + 4 * t) = xt;
                    double ss = (double)(xt.x * xt.x) + (double)(xt.y * xt.y) + (double)(xt.z * xt.z) + (double)(xt.w * xt.w);
                    ss = block_sum_d(ss, S.dscr);
                    const float scale = 1.0f / sqrtf((float)(ss / H) + p.eps);
                    const float4 wv = ldf4(p.tnw + 4 * t);
                    const float y0 = (xt.x * scale) * wv.x, y1 = (xt.y * scale) * wv.y, y2 = (xt.z * scale) * wv.z, y3 = (xt.w * scale) * wv.w;
                    uint2 hh2;
                    hh2.x = (uint32_t)f2h(y0) | ((uint32_t)f2h(y1) << 16);
                    hh2.y = (uint32_t)f2h(y2) | ((uint32_t)f2h(y3) << 16);
                    *reinterpret_cast<uint2 *>(p.txn + (size_t)b * H + 4 * t) = hh2;
                }
            }
        }
    }
    exit_ticket(reinterpret_cast<unsigned *>(p.state + SL.ctr), X.seq);
}

constexpr size_t LDS = lds_bytes<BLds>();

}  // namespace

size_t cpb_state_bytes() { return SL.total; }
bool cpb_error(const uint8_t *state, hipStream_t s, bool *err) { return state_error(SL, state, s, err); }
bool cpb_clear(uint8_t *state, hipStream_t s) { return state_clear(SL, state, s); }
bool cpb_resident(int device) {
    return resident<&k_cpb<1, false>, &k_cpb<2, false>>(device, LDS) && resident<&k_cpb<1, true>, &k_cpb<2, true>>(device, LDS);
}

bool persist_cp_batched(const CpbParams &p, hipStream_t s) {
    if (!p.L || !p.heads || !p.tabs || !p.out_norm || !p.qkvtab || !p.x_in || !p.rope || !p.pos || !p.kc || !p.vc || !p.logits ||
        !p.state || p.S < 1 || p.S > SMAX || p.sel.mode != SEL_CP || p.sel.V != CPV || !p.sel.tokens ||
        (p.talker_next && !(p.tx && p.txn && p.tnw && p.tr && p.tr_len && p.frame && p.pad))) {
        set_error("persist_cp_batched: bad parameters");
        return false;
    }
    if (p.sel.rec) return launch_by_tile_count<&k_cpb<1, true>, &k_cpb<2, true>>(p, LDS, s);
    return launch_by_tile_count<&k_cpb<1, false>, &k_cpb<2, false>>(p, LDS, s);
}

}  // namespace q3t
