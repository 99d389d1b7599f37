// persist_mm.h — the batched persistent launches' shared device machinery (persist_cpb.hip: the code-predictor frame,
// persist_tkb.hip: the talker step), 0.6B shapes, 1..64 slots:
//   - hand-offs: flags (sc1 payload stores, every storing wave's vmcnt(0), a workgroup barrier, one lane's sc1 flag
//     store; consumers poll with sc1 loads, then load the payload with sc1 loads) and {f32, tag} granules (one 8-byte
//     sc1 store, polled until every tag matches), both MI355X_MICROARCH.md hand-off table rows; bounded waits
//   - the MFMA tile job: 2 row tiles of 32 rows x one 32-token tile with k_gemm_mfma's numerics (gemm_mfma.hip): weights
//     DMA'd into LDS one job ahead, activations from hand-off buffers in B-fragment order, 4 K quarters summed in LDS
//   - the granule epilogue
//   - the decoder layer built on them, which both launches run: hand-off kinds and phase tags, the state layout, the
//     residual row's fold / norm_pub, the GEMM jobs (job_qkv / job_o / job_gu / job_dn / job_head), the weight issue one
//     job ahead, the selection's logits poll; and the host helpers of a launch (state error / clear, residency, launch)
// The .hip files keep their loop nest and job order, attention, selection commit and parameter check.
#pragma once
#include "persist.h"
#include "persist_dev.h"

namespace q3t {
namespace pmm {
using namespace pdev;

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

constexpr int H = 1024, NH = 16, NKV = 8, D = 128, QKVN = (NH + 2 * NKV) * D, INTER = 3072, CPV = 2048, VOC = 3072;
constexpr int G = 256, SMAX = 64;
constexpr int BUF_RSRC = 0x00020000;   // buffer resource word 3 (gfx9 family)
constexpr int SC1 = 16;                // buffer instruction cache policy: sc1
constexpr int SC1V = SC1 | (int)0x80000000u;   // sc1, volatile (a poll's load is re-issued every iteration)
constexpr int FLAGS_PER_KIND = 512;   // flag words per hand-off kind
constexpr int CTR_ERR = 32, CTR_TICKET = 48;   // counter words of the state block (StateLayout::ctr; seq is word 0)

// The f16 activation buffers behind flags (xna, xnf, attn, h) are kept in the MFMA B-fragment order of their consumers:
// 16-byte chunk k8 (halves 8 k8 .. 8 k8 + 7) of token tok at ((tok / 32 * kch + k8) * 32 + tok % 32) * 16 bytes, kch =
// K / 8.  A consumer wave's load instruction for chunk column (c, j) then reads two runs of 32 consecutive chunks (whole
// 64-byte sectors) instead of one 16-byte piece of 64 different sectors: sc1 loads are not merged in L1, so the
// row-major order moved every activation byte four times over the CU's L2 path.
__device__ __forceinline__ int fragoff(int kch, int tok, int k) {   // byte offset of half k of token tok (8-byte stores: k % 4 == 0)
    return (((tok >> 5) * kch + (k >> 3)) * 32 + (tok & 31)) * 16 + (k & 7) * 2;
}

struct Ctx {
    uint4 (*wl)[32][64];         // LDS: [wave][A slot][lane] (the next job's weight fragments / the K-quarter partials)
    uint64_t *prof;              // development timeline (null = off)
    Ctl c;
    unsigned seq;
    unsigned *flags;             // [kind][FLAGS_PER_KIND]
    __amdgpu_buffer_rsrc_t rs;   // the whole state block
    int S_;                      // slots
    __device__ uint32_t tag(int ph) const { return (seq << 10) + (unsigned)ph + 1u; }
    __device__ unsigned *flag(int kind, int j) const { return flags + kind * FLAGS_PER_KIND + j; }
};

// ---------------------------------------------------------------- flag polls
// every lane i < n of the wave polls flag idx(i); the wave leaves once all carry `tag` (bounded)
#ifdef Q3T_DEV
// development timeline (Q3T_PERSIST_PROF): thread 0 of each workgroup stamps phase ph, k = 0 wait start, 1 data ready,
// 2 published, 3 computed; [workgroup][768 phases][4] s_memrealtime (100 MHz)
#define CPROF(ph, k)                                                                                          \
    do {                                                                                                      \
        if (X.prof && threadIdx.x == 0) X.prof[((size_t)blockIdx.x * 768 + (ph)) * 4 + (k)] = wall_clock64(); \
    } while (0)
#else
#define CPROF(ph, k) ((void)0)
#endif
template <class Idx>
__device__ __forceinline__ void wait_flags(Ctx &X, int kind, int n, Idx idx, uint32_t tag) {
    const int lane = threadIdx.x & 63;
    const int ph_ = (int)((tag - 1u) & 1023u);
    (void)ph_;
    CPROF(ph_, 0);
    const unsigned *f0 = X.flags + kind * FLAGS_PER_KIND;
    const unsigned *fa = f0 + idx(lane < n ? lane : 0);
    const unsigned *fb = f0 + idx(lane + 64 < n ? lane + 64 : 0);
    unsigned it = 0;
    while (true) {
        bool ok = true;
        if (lane < n) ok &= __hip_atomic_load(fa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tag;
        if (lane + 64 < n) ok &= __hip_atomic_load(fb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tag;
        if (__all(ok) || X.c.abort) break;
        if (give_up(X.c, it)) break;
        __builtin_amdgcn_s_sleep(1);
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);   // the payload loads stay behind the poll
    CPROF(ph_, 1);
}

// the same for a whole workgroup: wave 0 polls every flag, the others load after the barrier it then joins (the polling
// traffic of one wave instead of four)
template <class Idx>
__device__ __forceinline__ void wait_flags_wg(Ctx &X, int kind, int n, Idx idx, uint32_t tag) {
    if (threadIdx.x < 64) wait_flags(X, kind, n, idx, tag);
    __syncthreads();
}

// publish: every storing wave drains its sc1 stores, then one lane signals for the workgroup
__device__ __forceinline__ void publish(Ctx &X, int kind, int j, uint32_t tag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(X.flag(kind, j), tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    CPROF((int)((tag - 1u) & 1023u), 2);
}

// the launch's LAST workgroup to finish bumps seq (ctr[0]; an exit ticket in ctr[CTR_TICKET]): every workgroup has read seq by
// then, whatever order the workgroups were dispatched in.  Every workgroup runs it, idle ones included
__device__ __forceinline__ void exit_ticket(unsigned *ctr, unsigned seq) {
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned *done = ctr + CTR_TICKET;
        if (__hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
            __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ctr, seq + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// spin until every granule a lane loads (issue(r) fills r) carries `tag` (bounded, as wait_flags)
template <int M, class Issue>
__device__ __forceinline__ void poll_gran(Ctx &X, uint32_t tag, u32x4_t (&r)[M], Issue issue) {
    unsigned it = 0;
    // gate: lane 0 alone polls its own granules first, so the wave's full sweeps start once the data is arriving
    if ((threadIdx.x & 63) == 0) {
        while (true) {
            issue(r);
            bool ok = true;
#pragma unroll
            for (int m = 0; m < M; ++m) ok &= r[m].y == tag && r[m].w == tag;
            if (ok || X.c.abort) break;
            if (give_up(X.c, it)) break;
            __builtin_amdgcn_s_sleep(1);
        }
    }
    X.c.abort = __shfl(X.c.abort ? 1 : 0, 0) != 0;
    it = 0;
    while (true) {
        issue(r);
        bool ok = true;
#pragma unroll
        for (int m = 0; m < M; ++m) ok &= r[m].y == tag && r[m].w == tag;
        if (__all(ok) || X.c.abort) break;
        if (give_up(X.c, it)) break;
        __builtin_amdgcn_s_sleep(1);
    }
}

// ---------------------------------------------------------------- MFMA tile job (gemm_mfma.hip k_gemm_mfma numerics)
// A job is RT = 2 row tiles of 32 rows (64 rows) x one 32-token tile: both row tiles share every activation fragment, so
// the activation rows every job pulls through the fabric (the sc1 hand-off reads, which bound these phases) are half
// those of 32-row jobs.  Per row tile the arithmetic is k_gemm_mfma's: A = W[row0 + 32 rt + r][k], B = X[token][k] for
// lane (r = lane & 31, h = lane >> 5), k = kq + 64c + 32h + 8j, wave w owning the K quarter kq = kbase + 64 NCH w, the
// MFMA chain in (c, j) order, the 4 quarters summed through LDS in wave order.
constexpr int RT = 2;
constexpr int RS = 68;   // row stride (floats) of the K-quarter partial tiles in LDS: the epilogue's 16-byte token-quad
                         // reads then fall on all 64 banks
template <int NCH>
__device__ __forceinline__ void load_w(uint4 (*wl)[32][64], const uint16_t *W, int ldw, int row0, int kbase) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
#ifdef CPB_EXP_NOW   // timing experiment (development variant builds): no weight loads
    return;
#endif
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const uint16_t *p = W + (size_t)(row0 + 32 * rt + r) * ldw + kbase + wave * (NCH * 64) + h * 32;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                __builtin_amdgcn_global_load_lds(p + c * 64 + j * 8, (__attribute__((address_space(3))) void *)&wl[wave][16 * rt + 4 * c + j][0],
                                                 16, 0, 0);
    }
}

// B fragments of tokens t0 + r: sc1 loads of the hand-off buffer at byte offset xoff (fragment order, kch chunks per
// token; the columns of tokens >= S read unwritten chunks and are never stored), then the MFMA chains; the K-quarter
// partials land in the wave's LDS region (its A slots, consumed)
template <int NCH>
__device__ __forceinline__ void mm_tile(Ctx &X, size_t xoff, int kch, int kbase, int t0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    u32x4_t xb[4 * NCH];
    const int off = (int)xoff + fragoff(kch, t0 + r, kbase + wave * (NCH * 64) + h * 32);
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#ifdef CPB_EXP_NOX   // timing experiment (development variant builds): no activation loads
            xb[4 * c + j] = u32x4_t{(unsigned)off, 0u, 0u, 0u};
#else
            xb[4 * c + j] = __builtin_amdgcn_raw_buffer_load_b128(X.rs, off + (c * 8 + j) * 512, 0, SC1);
#endif
        }
    f32x16_t acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[rt][i] = 0.0f;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's weight DMA (and the B fragments) have landed
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const half8_t bf = __builtin_bit_cast(half8_t, xb[4 * c + j]);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
                acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, X.wl[wave][16 * rt + 4 * c + j][lane]), bf,
                                                                 acc[rt], 0, 0, 0);
        }
    // every A slot this wave reads has been read (the MFMAs consumed them): the region takes the partials
    float *red = reinterpret_cast<float *>(&X.wl[wave][0][0]);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int i = 0; i < 16; ++i) red[(rt * 16 + i) * RS + lane] = acc[rt][i];
    __syncthreads();
}
// register i of row tile rt, lane `src`, summed over the 4 K quarters in wave order (k_gemm_mfma sum4)
__device__ __forceinline__ float sum4(const uint4 (*wl)[32][64], int rt, int i, int src) {
    float v = 0.0f;
#pragma unroll
    for (int w = 0; w < 4; ++w) v += reinterpret_cast<const float *>(&wl[w][0][0])[(rt * 16 + i) * RS + src];
    return v;
}

// granule epilogue (QKV rows, split-K slabs, lm_head logits): {f32, tag} granules out[tok][row0 ..] with 8-byte sc1
// stores (MI355X_MICROARCH.md handoff-1to1: the payload carries its own tag, no drain and no flag).  Thread t takes job
// row rho = t % 64 and the token quads 4 (t / 64) and 4 (t / 64) + 16: per wave 16-byte LDS reads of four tokens (8
// reads instead of 32 scalar ones: the epilogue is latency-bound at one wave per SIMD), and every store instruction
// writes 64 consecutive rows of one token (512 contiguous bytes).  Register i of lane (r, h) holds tile row
// (i & 3) + 8 (i >> 2) + 4h of token r, so row rr of a tile is register (rr & 3) + 4 (rr >> 3) of half (rr >> 2) & 1.
__device__ __forceinline__ void epi_gran(Ctx &X, size_t obase, int ldo, int row0, int t0, uint32_t tag) {
    const int t = threadIdx.x, rho = t & 63, tq = t >> 6;
    const int rt = rho >> 5, rr = rho & 31;
    const int src4 = ((rt * 16 + (rr & 3) + 4 * (rr >> 3)) * RS + 32 * ((rr >> 2) & 1)) / 4 + tq;   // 16-byte units
    uint4 q[2][4];   // all eight reads first (one LDS round trip), then the sums
#pragma unroll
    for (int hq = 0; hq < 2; ++hq)
#pragma unroll
        for (int w = 0; w < 4; ++w) q[hq][w] = (&X.wl[w][0][0])[src4 + 4 * hq];
#pragma unroll
    for (int hq = 0; hq < 2; ++hq) {
        const int r0 = 4 * tq + 16 * hq;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // k_gemm_mfma sum4: ((0 + q0) + q1) + q2) + q3
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            v[0] += __uint_as_float(q[hq][w].x); v[1] += __uint_as_float(q[hq][w].y);
            v[2] += __uint_as_float(q[hq][w].z); v[3] += __uint_as_float(q[hq][w].w);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {   // tokens S .. 63 too (rows of the SMAX-row buffer nobody reads): no branches
            const u32x2_t g = {__float_as_uint(v[u]), tag};
            __builtin_amdgcn_raw_buffer_store_b64(g, X.rs, (int)(obase + ((size_t)(t0 + r0 + u) * ldo + row0 + rho) * 8), 0, SC1);
        }
    }
    __syncthreads();   // the LDS region is the next job's DMA target
}

// ================================================================ the decoder layer both launches run
#pragma clang fp contract(off)   // every rounding as written: bit-identical to k_gemm_mfma / k_resid_norm

// hand-off kinds; a phase is (layer slot, kind): 8 per layer slot.  k_tkb's layer slots are its layers (28: the final
// norm / head), k_cpb's are 6 per pass (5: the final norm / head)
enum Kind { K_RNA = 0, K_QKV = 1, K_ATT = 2, K_O = 3, K_RNF = 4, K_GU = 5, K_DN = 6, K_HEAD = 7 };
__device__ __forceinline__ int ph_of(int ls, int k) { return ls * 8 + k; }

// ---------------------------------------------------------------- state block (zeroed once)
// xna / xnf / attn / h: f16 payloads behind flags; qkv, slo, sld, lg: {f32, tag} granules (8 B each, no flag); V = the
// logits width
struct StateLayout {
    size_t xna = 0;
    size_t xnf = xna + (size_t)SMAX * H * 2;
    size_t qkv = xnf + (size_t)SMAX * H * 2;
    size_t attn = qkv + (size_t)SMAX * QKVN * 8;
    size_t slo = attn + (size_t)SMAX * NH * D * 2;
    size_t sld = slo + (size_t)4 * SMAX * H * 8;
    size_t h = sld + (size_t)4 * SMAX * H * 8;
    size_t lg = h + (size_t)SMAX * INTER * 2;
    size_t flags;   // 8 kinds x FLAGS_PER_KIND u32
    size_t ctr;     // own lines: seq at ctr[0], the error word at ctr[32], the exit ticket at ctr[48]
    size_t total;
    constexpr explicit StateLayout(int V) : flags(lg + (size_t)SMAX * V * 8), ctr(flags + 8 * FLAGS_PER_KIND * 4), total(ctr + 256) {}
};
static_assert(StateLayout(CPV).flags == 8257536 && StateLayout(CPV).ctr == 8273920 && StateLayout(CPV).total == 8274176, "code-predictor state");
static_assert(StateLayout(VOC).flags == 8781824 && StateLayout(VOC).ctr == 8798208 && StateLayout(VOC).total == 8798464, "talker state");
static_assert(StateLayout(VOC).qkv == 262144 && StateLayout(VOC).attn == 2359296 && StateLayout(VOC).slo == 2621440 &&
              StateLayout(VOC).sld == 4718592 && StateLayout(VOC).h == 6815744 && StateLayout(VOC).lg == 7208960, "state offsets");

__device__ __forceinline__ Ctx make_ctx(uint8_t *state, const StateLayout &SL, uint64_t *prof, int S, uint4 (*wl)[32][64]) {
    unsigned *ctr = reinterpret_cast<unsigned *>(state + SL.ctr);
    return Ctx{wl, prof, Ctl{ctr + CTR_ERR, false}, __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
               reinterpret_cast<unsigned *>(state + SL.flags), __builtin_amdgcn_make_buffer_rsrc(state, 0, (int)SL.total, BUF_RSRC), S};
}

// ---------------------------------------------------------------- the residual row of slot b (thread t: x = elements 4t .. 4t+3)
// RMSNorm of x -> f16 row of slot b (fragment order) in the hand-off buffer `xo`, flag (kind, b); side (optional): the
// f32 normalised rows [slot][H]
__device__ __forceinline__ void norm_pub(Ctx &X, const float4 &x, int b, const float *nw, float eps, double *dscr, size_t xo, int kind,
                                         uint32_t tg, float *side) {
    const int t = threadIdx.x;
    double ss = (double)(x.x * x.x) + (double)(x.y * x.y) + (double)(x.z * x.z) + (double)(x.w * x.w);
    ss = block_sum_d(ss, dscr);
    const float scale = 1.0f / sqrtf((float)(ss / H) + eps);
    const float4 wv = ldf4(nw + 4 * t);
    const float y0 = (x.x * scale) * wv.x, y1 = (x.y * scale) * wv.y, y2 = (x.z * scale) * wv.z, y3 = (x.w * scale) * wv.w;
    if (side) *reinterpret_cast<float4 *>(side + (size_t)b * H + 4 * t) = make_float4(y0, y1, y2, y3);
    const u32x2_t hv = {(uint32_t)f2h(y0) | ((uint32_t)f2h(y1) << 16), (uint32_t)f2h(y2) | ((uint32_t)f2h(y3) << 16)};
    CPROF((int)((tg - 1u) & 1023u), 3);
    __builtin_amdgcn_raw_buffer_store_b64(hv, X.rs, (int)xo + fragoff(H / 8, b, 4 * t), 0, SC1);
    publish(X, kind, b, tg);
}
// x += the 4 split-K slabs of slot b (k_resid_norm<4> order): thread t polls the 16 granules of its 4 elements
__device__ __forceinline__ void fold(Ctx &X, float4 &x, int b, size_t slab, uint32_t tg) {
    const int t = threadIdx.x;
    const int ph_ = (int)((tg - 1u) & 1023u);
    (void)ph_;
    CPROF(ph_, 0);
    u32x4_t pz[8];
    poll_gran<8>(X, tg, pz, [&](u32x4_t (&r)[8]) {
#pragma unroll
        for (int z = 0; z < 4; ++z)
#pragma unroll
            for (int hh2 = 0; hh2 < 2; ++hh2)
                r[2 * z + hh2] = __builtin_amdgcn_raw_buffer_load_b128(X.rs, (int)(slab + (((size_t)z * SMAX + b) * H + 4 * t + 2 * hh2) * 8), 0, SC1V);
    });
    CPROF(ph_, 1);
#pragma unroll
    for (int z = 0; z < 4; ++z)
        x = make_float4(x.x + __uint_as_float(pz[2 * z].x), x.y + __uint_as_float(pz[2 * z].z), x.z + __uint_as_float(pz[2 * z + 1].x),
                        x.w + __uint_as_float(pz[2 * z + 1].z));
}

// ---------------------------------------------------------------- GEMM jobs (64 rows x the 32 tokens of tile tt; ls = the layer slot)
// full-K job j (row panel j % nrp, tile j / nrp) on the normalised rows xna: granules out[tok][64 rp ..] of kind `kout`
__device__ __forceinline__ void job_rows(Ctx &X, const StateLayout &SL, int j, int nrp, int ls, int kout, size_t obase, int ldo) {
    const int rp = j % nrp, tt = j / nrp;
    const int nv = min(32, X.S_ - 32 * tt);
    wait_flags_wg(X, K_RNA, nv, [&](int i) { return 32 * tt + i; }, X.tag(ph_of(ls, K_RNA)));
    mm_tile<4>(X, SL.xna, H / 8, 0, 32 * tt);
    CPROF(ph_of(ls, kout), 3);
    epi_gran(X, obase, ldo, 64 * rp, 32 * tt, X.tag(ph_of(ls, kout)));
    CPROF(ph_of(ls, kout), 2);
}
__device__ __forceinline__ void job_qkv(Ctx &X, const StateLayout &SL, int w, int ls) { job_rows(X, SL, w, 64, ls, K_QKV, SL.qkv, QKVN); }
// lm_head / codec head: V logits, nrp = V / 64 row panels
__device__ __forceinline__ void job_head(Ctx &X, const StateLayout &SL, int w, int ls, int V, int nrp) {
    job_rows(X, SL, w, nrp, ls, K_HEAD, SL.lg, V);
}
// O: split-K slab z (heads 4z .. 4z+3) of rows 64 rp .. +63; wait(z, tt, nv, tag) returns once the tile's attention
// rows of that slice are published
template <class Wait>
__device__ __forceinline__ void job_o(Ctx &X, const StateLayout &SL, int w, int ls, Wait wait) {
    const int rp = w % 16, z = (w / 16) % 4, tt = w / 64;
    const int nv = min(32, X.S_ - 32 * tt);
    wait(z, tt, nv, X.tag(ph_of(ls, K_ATT)));
    mm_tile<2>(X, SL.attn, NH * D / 8, 512 * z, 32 * tt);
    CPROF(ph_of(ls, K_O), 3);
    epi_gran(X, SL.slo + (size_t)z * SMAX * H * 8, H, 64 * rp, 32 * tt, X.tag(ph_of(ls, K_O)));
    CPROF(ph_of(ls, K_O), 2);
}
// GU: 32 SwiGLU units (rows 64 rp .. +63, gate/up interleaved in 16-row blocks) -> h f16, flag (K_GU, gj)
__device__ __forceinline__ void job_gu(Ctx &X, const StateLayout &SL, int gj, int ls) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rp = gj % 96, tt = gj / 96;
    const int nv = min(32, X.S_ - 32 * tt);
    wait_flags_wg(X, K_RNF, nv, [&](int i) { return 32 * tt + i; }, X.tag(ph_of(ls, K_RNF)));
    mm_tile<4>(X, SL.xnf, H / 8, 0, 32 * tt);
    CPROF(ph_of(ls, K_GU), 3);
    {   // k_gemm_mfma SWIGLU epilogue per row tile: wave = (rt, q)
        const int rt = wave >> 1, q = wave & 1, r = lane & 31, h = lane >> 5;
        const int tok = 32 * tt + r;
        if (tok < X.S_) {
            const int unit = 32 * rp + 16 * rt + 8 * q + 4 * h;
            float hv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) hv[e] = silu_f(sum4(X.wl, rt, 4 * q + e, lane)) * sum4(X.wl, rt, 4 * (q + 2) + e, lane);
            const u32x2_t o = {(uint32_t)f2h(hv[0]) | ((uint32_t)f2h(hv[1]) << 16), (uint32_t)f2h(hv[2]) | ((uint32_t)f2h(hv[3]) << 16)};
            __builtin_amdgcn_raw_buffer_store_b64(o, X.rs, (int)SL.h + fragoff(INTER / 8, tok, unit), 0, SC1);
        }
    }
    publish(X, K_GU, gj, X.tag(ph_of(ls, K_GU)));
}
// DN: split-K slab z of rows 64 rp .. +63; wave v reads units [768 z + 192 v, +192)
__device__ __forceinline__ void job_dn(Ctx &X, const StateLayout &SL, int w, int ls) {
    const int wave = threadIdx.x >> 6;
    const int rp = w % 16, z = (w / 16) % 4, tt = w / 64;
    // each wave waits for the 6 gate/up jobs of its own K quarter only (units [768 z + 192 v, +192)): no barrier, no wave
    // held by another quarter's late producer
    wait_flags(X, K_GU, 6, [&](int i) { return 24 * z + 6 * wave + i + 96 * tt; }, X.tag(ph_of(ls, K_GU)));
    mm_tile<3>(X, SL.h, INTER / 8, 768 * z, 32 * tt);
    CPROF(ph_of(ls, K_DN), 3);
    epi_gran(X, SL.sld + (size_t)z * SMAX * H * 8, H, 64 * rp, 32 * tt, X.tag(ph_of(ls, K_DN)));
    CPROF(ph_of(ls, K_DN), 2);
}

// ---------------------------------------------------------------- weight issue, one job ahead
// The workgroup's job classes: QKV / O / DN jobs on workgroups [0, 64 NT), lm_head on [0, nhp NT) (nhp row panels), and
// gate/up job gj on workgroups [0, 128), then the odd slot workgroups 129, 131, ...: the residual rows' workgroups
// (even) run the norm right before gate/up, so a gate/up job there started ~2 us after the others
constexpr int SW0 = 128;   // slot workgroups: SW0 + 2b (slot b's residual row) and SW0 + 2b + 1
struct Jobs {
    int w, gj;
    bool hq, hg, hh, slot;
    __device__ __forceinline__ Jobs(int w_, int NT, int nhp, int S)
        : w(w_), gj(w_ < SW0 ? w_ : (w_ & 1) ? SW0 + (w_ - SW0 - 1) / 2 : -1), hq(w_ < 64 * NT), hg(gj >= 0 && gj < 96 * NT), hh(w_ < nhp * NT),
          slot(w_ >= SW0 && w_ - SW0 < 2 * S) {}
    __device__ __forceinline__ bool has(int k) const { return k == K_GU ? hg : k == K_HEAD ? hh : hq; }
};
struct WJob { int pass = 0, l = 0, k = K_QKV; };   // the job whose weights wl holds: (pass, layer or nl = the head, kind)
// Advance: (WJob &) -> the kernel's next job in program order (pass >= npass: none left); HeadW: (const WJob &) -> the
// head job's weights
template <class Advance, class HeadW>
struct WeightIssue {
    uint4 (*wl)[32][64];
    const PLayerW *layers;   // [nl]
    int nl, npass, nhp;
    Jobs J;
    Advance advance;
    HeadW head;
    WJob j;
    bool pending = false;
    __device__ __forceinline__ void issue() {
        while (j.pass < npass && !J.has(j.k)) advance(j);
        if (j.pass >= npass) return;
        const PLayerW &Lw = layers[j.l < nl ? j.l : 0];
        const int w = J.w;
        switch (j.k) {
            case K_QKV: load_w<4>(wl, Lw.qkv, H, 64 * (w % 64), 0); break;
            case K_O: load_w<2>(wl, Lw.o, NH * D, 64 * (w % 16), 512 * ((w / 16) % 4)); break;
            case K_GU: load_w<4>(wl, Lw.gu, H, 64 * (J.gj % 96), 0); break;
            case K_DN: load_w<3>(wl, Lw.down, INTER, 64 * (w % 16), 768 * ((w / 16) % 4)); break;
            default: load_w<4>(wl, head(j), H, 64 * (w % nhp), 0); break;
        }
    }
    __device__ __forceinline__ void next_job() { advance(j); issue(); }
    // a slot workgroup issues the next job's weights after its next attention (the polls of the norm and attention steps
    // before it then do not queue behind 128 KB of weight DMA), at the latest when that job starts: defer, then flush
    __device__ __forceinline__ void defer() { pending = true; }
    __device__ __forceinline__ void after_job() { if (J.slot) pending = true; else next_job(); }
    __device__ __forceinline__ void flush() { if (pending) { next_job(); pending = false; } }
};
template <class Advance, class HeadW>
__device__ __forceinline__ WeightIssue<Advance, HeadW> weight_issue(uint4 (*wl)[32][64], const PLayerW *layers, int nl, int npass, int nhp,
                                                                    const Jobs &J, Advance advance, HeadW head) {
    return WeightIssue<Advance, HeadW>{wl, layers, nl, npass, nhp, J, advance, head};
}

// ---------------------------------------------------------------- selection input
// thread t polls logits VPT t .. VPT t + VPT - 1 of slot b's row (select_token's exact-width ownership, V = 256 VPT)
// into v[], padded with -inf
template <int VPT, int NV>
__device__ __forceinline__ void poll_logits(Ctx &X, size_t lg, int b, uint32_t tg, float (&v)[NV]) {
    const int t = threadIdx.x;
    u32x4_t lr[VPT / 2];
    poll_gran<VPT / 2>(X, tg, lr, [&](u32x4_t (&r)[VPT / 2]) {
#pragma unroll
        for (int k = 0; k < VPT / 2; ++k)
            r[k] = __builtin_amdgcn_raw_buffer_load_b128(X.rs, (int)(lg + ((size_t)b * (VPT * 256) + VPT * t + 2 * k) * 8), 0, SC1V);
    });
#pragma unroll
    for (int k = 0; k < VPT / 2; ++k) { v[2 * k] = __uint_as_float(lr[k].x); v[2 * k + 1] = __uint_as_float(lr[k].z); }
#pragma unroll
    for (int e = VPT; e < NV; ++e) v[e] = -INFINITY;
}

// ================================================================ host side of a batched launch
// K1 / K2: the kernel's instantiations for one / two token tiles; SL: its state layout
template <class Lds>
constexpr size_t lds_bytes() {
    static_assert(sizeof(Lds) <= 160 * 1024, "LDS");
    return std::max(sizeof(Lds), (size_t)96 * 1024);   // > 80 KB: one workgroup per CU
}
template <auto K>
bool attr(size_t lds) {
    static bool done = false;
    if (!done) {
        Q3T_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        done = true;
    }
    return true;
}
template <auto K1, auto K2>
bool resident(int device, size_t lds) {   // both instantiations fit one workgroup per CU, >= G CUs
    int n_cu = 0, blocks = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n_cu < G) return false;
    for (const void *k : {reinterpret_cast<const void *>(K1), reinterpret_cast<const void *>(K2)}) {
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k, 256, lds) != hipSuccess || blocks < 1) return false;
    }
    return true;
}
template <auto K1, auto K2, class P>
bool launch_by_tile_count(const P &p, size_t lds, hipStream_t s) {
    if (p.S <= 32) {
        if (!attr<K1>(lds)) return false;
        hipLaunchKernelGGL(K1, dim3(G), dim3(256), lds, s, p);
    } else {
        if (!attr<K2>(lds)) return false;
        hipLaunchKernelGGL(K2, dim3(G), dim3(256), lds, s, p);
    }
    Q3T_HIP(hipGetLastError());
    return true;
}
inline bool state_error(const StateLayout &SL, const uint8_t *state, hipStream_t s, bool *err) {
    unsigned e = 0;
    Q3T_HIP(hipMemcpyAsync(&e, state + SL.ctr + CTR_ERR * 4, 4, hipMemcpyDeviceToHost, s));
    Q3T_HIP(hipStreamSynchronize(s));
    *err = e != 0;
    return true;
}
inline bool state_clear(const StateLayout &SL, uint8_t *state, hipStream_t s) {   // after a fault: zero the flags and the error word (seq kept)
    Q3T_HIP(hipMemsetAsync(state + SL.flags, 0, SL.ctr - SL.flags, s));
    Q3T_HIP(hipMemsetAsync(state + SL.ctr + CTR_ERR * 4, 0, 4, s));
    Q3T_HIP(hipMemsetAsync(state + SL.ctr + CTR_TICKET * 4, 0, 4, s));   // the exit ticket
    return true;
}

}  // namespace pmm
}  // namespace q3t
