// persist_roles.h — what the two one-slot role kernels share (persist_tk.hip k_tk_roles: the talker step;
// persist_cp.hip k_cp_roles: the code-predictor frame), 0.6B shapes: the role context with its phase tags, the
// development-timeline stamp, and the GEMV role bodies over a role's register-held weights -- QKV rows, head rows,
// gate/up + SwiGLU, down + residual.  Every body keeps the per-op GEMVs' lane split and reduction order (gemv.hip), so
// both kernels stay bit-identical to the launch-per-op graph through this one copy.
// Each .hip keeps its role-to-workgroup map, LDS struct, loop nest (which layer or head is issued next), the way a
// phase's input row is obtained, its O role, attention and selection.  What differs in a shared body comes in through
// a policy type P of the including kernel, never through a Q3T_TK_* / Q3T_CP_* macro:
//   P::WPUB       QKV phase: each wave publishes its own 16 rows (false: through LDS, wave 0 publishes all 64)
//   P::PUT_FIRST  a barrier after a role's publish, so the next weight prefetch enters the CU's memory pipe behind it
//   P::GATE       polls: lane 0 of each wave gates on the wave's first granule before the sweep
//   P::wait<N>    the sweep of N contiguous granules (g_waitc)
//   P::ldw        the 16-byte weight load (ld16; ld_nt16 where every row is read once per launch by one CU)
// Include this header after the .hip's `#pragma clang fp contract(off)`; the pragma is repeated here because the
// bodies must round as written.
#pragma once
#include "persist_dev.h"

#pragma clang fp contract(off)

#ifndef Q3T_QKV_SCATTER   // WPUB publish, 1: the row sums by reduce-scatter and row swaps (0: 16 adds and four ds_bpermute)
#define Q3T_QKV_SCATTER 0
#endif

namespace q3t {
namespace prole {
using namespace pdev;

constexpr int H = 1024, NH = 16, NKV = 8, D = 128, QKVN = (NH + 2 * NKV) * D, INTER = 3072;

// p: the launch's parameters; S: the kernel's LDS struct (xs, xr, red, outv, dscr, hs are the members used here)
template <class LDS>
struct RoleCtx {
    const PersistParams &p;
    LDS &S;
    Ctl c;
    unsigned seq;
    __device__ uint32_t tag(int ph) const { return ((seq * 1024u + (unsigned)ph) << 1) | 1u; }
};

// development timeline (p.prof): wall clock at k = 0 wait start / 1 input arrived / 2 output published / 3 mid-phase.
// Only the development and experiment builds (Q3T_DEV) allocate p.prof; in the release library the stamp is no code
// (each one was a test of p.prof and a branch on the chain, 3-4 per role body).
#ifdef Q3T_DEV
#define PROF(ph, k)                                                                                           \
    do {                                                                                                      \
        if (X.p.prof && threadIdx.x == 0 && blockIdx.x < PROF_WG) X.p.prof[((size_t)blockIdx.x * PROF_PH + (ph)) * 4 + (k)] = wall_clock64(); \
    } while (0)
#else
#define PROF(ph, k) ((void)0)
#endif

// a role's input poll: N contiguous granules at g, behind the one-lane gate
template <class P, int N, class C>
__device__ __forceinline__ void wait_in(C &X, const uint64_t *g, uint32_t tag, uint32_t (&u)[N]) {
    if (P::GATE) g_gate(g, tag, X.c);
    P::template wait<N>(g, tag, u, X.c);
}
// the end of every role phase: stamp the publish, then (PUT_FIRST) hold the other waves' prefetch behind wave 0's store
template <class P, class C>
__device__ __forceinline__ void published(C &X, int ph) {
    PROF(ph, 2);
    if (P::PUT_FIRST) __syncthreads();
}

// 16-lane-group row over K = 1024: lane l16 holds k = l16 * 8 + tt * 128, tt < 8 (two K halves of 4)
template <class P>
__device__ __forceinline__ void issue_row(const uint16_t *W, int row, uint4 (&w)[8]) {
    const uint16_t *r = W + (size_t)row * H + (threadIdx.x & 15) * 8;
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) w[tt] = P::ldw(r + tt * 128);
}

// ------------------------------------------------------------------ QKV rows 64i .. 64i + 63 (4 x 16)
template <class P>
__device__ __forceinline__ void qkv_issue(const uint16_t *W, const float *norm, int i, uint4 (&wq)[4][8], float4 &nw) {
    const int t = threadIdx.x, grp = t >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j)   // WPUB: wave w owns rows 16w .. 16w + 15 (row 16w + 4j + lane / 16) and publishes them itself
        issue_row<P>(W, 64 * i + (P::WPUB ? 16 * (t >> 6) + 4 * j + (grp & 3) : 16 * j + grp), wq[j]);
    nw = ldf4(norm + 4 * t);
}
// RMSNorm(nw) of x (elements 4t..4t+3) -> the 64 rows -> gqkv, tagged ph
template <class P, class C>
__device__ __forceinline__ void qkv_phase(C &X, int i, float4 x, const uint4 (&wq)[4][8], float4 nw, int ph) {
    auto &S = X.S;
    const int t = threadIdx.x, l16 = t & 15, grp = t >> 4;
    rms_to_f16(x, nw, X.p.eps, S.xs, S.dscr, nullptr);
    __syncthreads();
    float acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acc[j] = 0.0f;
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) acc[j] = dot8(wq[j][tt], *reinterpret_cast<const uint4 *>(S.xs + l16 * 8 + tt * 128), acc[j]);
    }
    if constexpr (P::WPUB) {
        // each wave publishes its 16 rows as one whole line, no barrier
        const int lane = t & 63;
        if constexpr (Q3T_QKV_SCATTER) {
            // the four row sums of every 16-lane group as one reduce-scatter (group_sum<16>'s tree per row, 5 adds for
            // 16), then lane L < 16 takes group L / 4's value at its own lane position over two row swaps: that is row
            // 4j + L / 4, j = scatter4_index(L), so the same one store writes the line's granules in a permuted order.
            // Measured and not faster (DESIGN 2a''): off
            const float pv = rows_gather16(group16_sum_scatter4(acc));
            if (lane < 16)
                g_put(X.p.gqkv + 64 * i + 16 * (t >> 6) + 4 * scatter4_index(lane) + (lane >> 2), __float_as_uint(pv), X.tag(ph));
        } else {   // lane L < 16 takes row 4j + g (j = L / 4, g = L % 4) from lane 16 g of the group that reduced it
            float pv = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = __shfl(group_sum<16>(acc[j]), 16 * (lane & 3));
                if ((lane >> 2) == j) pv = v;
            }
            if (lane < 16) g_put(X.p.gqkv + 64 * i + 16 * (t >> 6) + lane, __float_as_uint(pv), X.tag(ph));
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[j] = group_sum<16>(acc[j]);
            if (l16 == 0) S.outv[16 * j + grp] = acc[j];
        }
        __syncthreads();
        // one store instruction of wave 0 publishes the 64 rows (4 whole lines): single-lane stores from four waves
        // into shared lines make the next edge slower
        if (t < 64) g_put(X.p.gqkv + 64 * i + t, __float_as_uint(S.outv[t]), X.tag(ph));
    }
    published<P>(X, ph);
}

// ------------------------------------------------------------------ head rows: NJ groups of 16 over the f16 tile S.xs
// row 16j + grp of the workgroup's block (wq[j], issue_row) as two K halves, (half 0) + (half 1), into S.outv; the
// caller runs the barrier and publishes
template <int NJ, class C>
__device__ __forceinline__ void head_rows(C &X, const uint4 (&wq)[4][8]) {
    auto &S = X.S;
    const int t = threadIdx.x, l16 = t & 15, grp = t >> 4;
    float a0[NJ], a1[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        a0[j] = 0.0f;
        a1[j] = 0.0f;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) a0[j] = dot8(wq[j][tt], *reinterpret_cast<const uint4 *>(S.xs + l16 * 8 + tt * 128), a0[j]);
#pragma unroll
        for (int tt = 4; tt < 8; ++tt) a1[j] = dot8(wq[j][tt], *reinterpret_cast<const uint4 *>(S.xs + l16 * 8 + tt * 128), a1[j]);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const float lg = group_sum<16>(a0[j]) + group_sum<16>(a1[j]);
        if (l16 == 0) S.outv[16 * j + grp] = lg;
    }
}

// ------------------------------------------------------------------ gate/up + SwiGLU units 32i .. 32i + 31 (2 x 16)
// unit 32i + 16j + grp: gate row, up row 16 below (16-row interleaved blocks)
template <class P>
__device__ __forceinline__ void gu_issue(const uint16_t *W, const float *norm, int i, uint4 (&wg)[2][8], uint4 (&wu)[2][8], float4 &nw) {
    const int t = threadIdx.x, grp = t >> 4;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int unit = 32 * i + 16 * j + grp, row = (unit >> 4) * 32 + (unit & 15);
        issue_row<P>(W, row, wg[j]);
        issue_row<P>(W, row + 16, wu[j]);
    }
    nw = ldf4(norm + 4 * t);
}
// RMSNorm(nw) of x (elements 4t..4t+3) -> the 32 units -> gh (f16 pairs), tagged ph
template <class P, class C>
__device__ __forceinline__ void gu_phase(C &X, int i, float4 x, const uint4 (&wg)[2][8], const uint4 (&wu)[2][8], float4 nw, int ph) {
    auto &S = X.S;
    const int t = threadIdx.x, l16 = t & 15, grp = t >> 4;
    rms_to_f16(x, nw, X.p.eps, S.xs, S.dscr, nullptr);
    __syncthreads();
    float a0[2], a1[2], b0[2], b1[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        a0[j] = a1[j] = b0[j] = b1[j] = 0.0f;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const uint4 xv = *reinterpret_cast<const uint4 *>(S.xs + l16 * 8 + tt * 128);
            a0[j] = dot8(wg[j][tt], xv, a0[j]);
            b0[j] = dot8(wu[j][tt], xv, b0[j]);
        }
#pragma unroll
        for (int tt = 4; tt < 8; ++tt) {
            const uint4 xv = *reinterpret_cast<const uint4 *>(S.xs + l16 * 8 + tt * 128);
            a1[j] = dot8(wg[j][tt], xv, a1[j]);
            b1[j] = dot8(wu[j][tt], xv, b1[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float ga = group_sum<16>(a0[j]) + group_sum<16>(a1[j]);
        const float ub = group_sum<16>(b0[j]) + group_sum<16>(b1[j]);
        if (l16 == 0) S.hs[16 * j + grp] = silu_f(ga) * ub;
    }
    __syncthreads();
    if (t < 16) g_put(X.p.gh + 16 * i + t, (uint32_t)f2h(S.hs[2 * t]) | ((uint32_t)f2h(S.hs[2 * t + 1]) << 16), X.tag(ph));
    published<P>(X, ph);
}

// ------------------------------------------------------------------ down rows lo .. lo + n - 1 (n <= 20, 5 x 4) + residual
// row lo + 4j + grp4 (clamped: rows past n re-read row lo + n - 1), K slice = wave (k_gemv<1,1,4,PRO_F16,8>)
template <class P>
__device__ __forceinline__ void dn_issue(const uint16_t *W, int lo, int n, uint4 (&wd)[5][6]) {
    const int t = threadIdx.x, wave = t >> 6, grp4 = (t & 63) >> 4;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint16_t *r = W + (size_t)(lo + min(4 * j + grp4, n - 1)) * INTER + wave * 768 + (t & 15) * 8;
#pragma unroll
        for (int tt = 0; tt < 6; ++tt) wd[j][tt] = P::ldw(r + tt * 128);
    }
}
// h (gh, tagged ph - 1: the gate/up phase of the same layer) -> the rows' four K-slice sums through S.red[par] ->
// S.xr[t] + ((s0 + s1) + s2) + s3 -> gx, tagged ph.  The caller has filled S.xr[0 .. n) and alternates par.
template <class P, class C>
__device__ __forceinline__ void dn_phase(C &X, int lo, int n, int par, const uint4 (&wd)[5][6], int ph) {
    auto &S = X.S;
    const int t = threadIdx.x, wave = t >> 6, l16 = t & 15, grp4 = (t & 63) >> 4;
    uint32_t u[6];
    PROF(ph, 0);
    wait_in<P, 6>(X, X.p.gh + 6 * t, X.tag(ph - 1), u);
    PROF(ph, 1);
    *reinterpret_cast<uint2 *>(S.xs + 12 * t) = make_uint2(u[0], u[1]);
    *reinterpret_cast<uint2 *>(S.xs + 12 * t + 4) = make_uint2(u[2], u[3]);
    *reinterpret_cast<uint2 *>(S.xs + 12 * t + 8) = make_uint2(u[4], u[5]);
    wave_lds_sync();   // wave w polled exactly the K slice [768 w, 768 w + 768) it multiplies
    float acc[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        acc[j] = 0.0f;
#pragma unroll
        for (int tt = 0; tt < 6; ++tt)
            acc[j] = dot8(wd[j][tt], *reinterpret_cast<const uint4 *>(S.xs + wave * 768 + l16 * 8 + tt * 128), acc[j]);
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        acc[j] = group_sum<16>(acc[j]);
        if (l16 == 0) S.red[par][wave][4 * j + grp4] = acc[j];
    }
    __syncthreads();
    if (t < n) {
        const float (&rd)[4][32] = S.red[par];
        const float s = rd[0][t] + rd[1][t] + rd[2][t] + rd[3][t];
        g_put(X.p.gx + lo + t, __float_as_uint(S.xr[t] + s), X.tag(ph));
    }
    published<P>(X, ph);
}

}  // namespace prole
}  // namespace q3t
