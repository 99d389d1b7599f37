// kernels.hip — hand-written gfx950 (CDNA4) kernels of the per-frame decode path.
//
// Numerics follow the reference CPU path (GGML_CUDA=OFF): f16 weights exactly as stored in the GGUF, every
// matmul input activation rounded to f16 (ggml mul_mat converts src1 to vec_dot_type F16), products
// accumulated in f32 (v_dot2_f32_f16: exact f16 products), F16 KV cache, f32 norms/softmax/residuals.
#include "kernels.h"
#include "select.h"

#include <algorithm>

namespace q3t {

// ======================================================================================= token selection
// REC: the slots' sampling records (sp.rec, per-utterance sampling); launched without it when sp.rec is null
template <bool REC>
__global__ void __launch_bounds__(256) k_select(const SelectSpec sp, const float *logits) {
    __shared__ SelLds S;
    select_slot<false, REC>(sp, logits + (size_t)blockIdx.x * sp.V, blockIdx.x, S);
}
bool select_tokens(const SelectSpec &sp, const float *logits, int S, hipStream_t s) {
    if (sp.V > 256 * SEL_VPT_MAX || sp.V <= 0) { set_error("select: vocab must be in (0, 4096]"); return false; }
    if (S <= 0) return true;
    if (sp.rec) hipLaunchKernelGGL(k_select<true>, dim3(S), dim3(256), 0, s, sp, logits);
    else hipLaunchKernelGGL(k_select<false>, dim3(S), dim3(256), 0, s, sp, logits);
    Q3T_HIP(hipGetLastError());
    return true;
}

// GatherSum rows materialised (batched path: the matrix-core GEMM has no gather prologue).  Same order of the f32
// sums as gemv.hip's issue_x_gather, so both paths see bit-identical activation rows.
template <int NT>
__global__ void __launch_bounds__(256) k_gather_sum(const GatherSum gs, int K, float *out, int ldo) {
    const int b = blockIdx.x;
    for (int k = threadIdx.x * 4; k < K; k += 1024) {   // K > 1024 (1.7B talker rows): one 1024-wide chunk per pass
    const uint16_t *row[NT];
    const float *extra = nullptr;
    if constexpr (NT == 1) {
        row[0] = gs.tab0 + (size_t)gs.tok[(size_t)b * gs.tok_ld + gs.tok_col0] * K;
    } else {
        const int *tk = gs.tok + (size_t)b * gs.tok_ld;
#pragma unroll
        for (int j = 0; j < NT; ++j) row[j] = gs.tabs[j] + (size_t)tk[j] * K;
        const int fr = gs.frame[b];
        extra = fr < gs.tr_len[b] ? gs.tr + (size_t)b * gs.tr_ld + (size_t)fr * K : gs.pad + (size_t)b * K;
    }
    float a[4];
    {
        const uint2 u = *reinterpret_cast<const uint2 *>(row[0] + k);
        a[0] = h2f(u.x & 0xffff); a[1] = h2f(u.x >> 16); a[2] = h2f(u.y & 0xffff); a[3] = h2f(u.y >> 16);
    }
#pragma unroll
    for (int j = 1; j < NT; ++j) {
        const uint2 u = *reinterpret_cast<const uint2 *>(row[j] + k);
        a[0] += h2f(u.x & 0xffff); a[1] += h2f(u.x >> 16); a[2] += h2f(u.y & 0xffff); a[3] += h2f(u.y >> 16);
    }
    if constexpr (NT > 1) {
        const float4 e = *reinterpret_cast<const float4 *>(extra + k);
        a[0] += e.x; a[1] += e.y; a[2] += e.z; a[3] += e.w;
    }
    *reinterpret_cast<float4 *>(out + (size_t)b * ldo + k) = make_float4(a[0], a[1], a[2], a[3]);
    }
}
bool gather_sum(const GatherSum &gs, int nt, int S, int K, float *out, int ldo, hipStream_t s) {
    if (K % 4 != 0 || (nt != 1 && nt != 16)) { set_error("gather_sum: unsupported shape"); return false; }
    if (S <= 0) return true;
    if (nt == 1) hipLaunchKernelGGL(k_gather_sum<1>, dim3(S), dim3(256), 0, s, gs, K, out, ldo);
    else hipLaunchKernelGGL(k_gather_sum<16>, dim3(S), dim3(256), 0, s, gs, K, out, ldo);
    Q3T_HIP(hipGetLastError());
    return true;
}

// a slot whose utterance ended (done >= 0) stays where it is: its position never runs past the context reserved
// for it, however long the other slots (or a continuous-batching queue) keep the frame loop going
__global__ void k_advance(int *pos, int *frame, const int *done, int S) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S && !(done && done[s] >= 0)) { pos[s] += 1; frame[s] += 1; }
}
bool advance(int *pos, int *frame, const int *done, int S, hipStream_t s) {
    hipLaunchKernelGGL(k_advance, dim3((S + 63) / 64), dim3(64), 0, s, pos, frame, done, S);
    Q3T_HIP(hipGetLastError());
    return true;
}

// One workgroup (one wave) per slot.  A slot's complete frames: the EOS frame index once it ended (select_commit sets
// done to the frame whose CB0 was EOS, and that frame is not part of the utterance), otherwise the frame counter,
// which k_advance and the fused advance of k_tkb / k_cpb raise only after all 16 codes of the frame are written.
// The header entry and the counter are written after every lane has read the counter (one wave: program order).
__global__ void __launch_bounds__(64) k_queue_collect(const QueueCollect q) {
    const int k = blockIdx.x;
    if (!q.mask[k]) return;
    const int done = q.done[k], delivered = q.delivered[k];
    const int cap = q.slot_max_len ? min(q.slot_max_len[k], q.max_len) : q.max_len;   // (<= codes_max_len: the rows read)
    const int avail = min(done >= 0 ? done : q.frame[k], cap);
    const int n = avail - delivered;
    if (delivered < 0 || n < 0 || n > q.interval) {   // never expected: nothing is copied, the host sees the word
        if (threadIdx.x == 0) { *q.error = 1; q.header[k] = 0; }
        return;
    }
    const int4 *src = reinterpret_cast<const int4 *>(q.codes + ((size_t)k * q.codes_max_len + delivered) * 16);
    int4 *dst = reinterpret_cast<int4 *>(q.rows + (size_t)k * q.interval * 16);
    for (int i = threadIdx.x; i < n * 4; i += 64) dst[i] = src[i];   // a row is 4 x 16 bytes
    if (threadIdx.x == 0) { q.header[k] = n; q.delivered[k] = avail; }
}
bool queue_collect(const QueueCollect &q, int S, hipStream_t s) {
    if (S <= 0) return true;
    if (q.interval <= 0 || q.max_len < 0 || q.max_len > q.codes_max_len) { set_error("queue_collect: bad shape"); return false; }
    hipLaunchKernelGGL(k_queue_collect, dim3(S), dim3(64), 0, s, q);
    Q3T_HIP(hipGetLastError());
    return true;
}

// ------------------------------------------------------------------------------------------ text feeds
// Workgroups [0, n_rows) copy one projected row each into its slot's trailing buffer; the last workgroup publishes
// the counters.  Nothing in this launch reads what another workgroup of it writes: the next frame's gather does.
__global__ void __launch_bounds__(256) k_text_append(const TextAppend t) {
    const int b = blockIdx.x;
    if (b < t.n_rows) {
        const int src = t.rows[3 * b], slot = t.rows[3 * b + 1], dst = t.rows[3 * b + 2];
        if (src < 0 || src >= t.src_rows || slot < 0 || slot >= t.S || dst < 0 || dst >= t.max_trailing) {
            if (threadIdx.x == 0) *t.error = 1;
            return;
        }
        const float4 *from = reinterpret_cast<const float4 *>(t.src + (size_t)src * t.H);
        float4 *to = reinterpret_cast<float4 *>(t.trailing + ((size_t)slot * t.max_trailing + dst) * t.H);
        for (int i = threadIdx.x; i < t.H / 4; i += 256) to[i] = from[i];
        return;
    }
    for (int j = threadIdx.x; j < t.n_commit; j += 256) {
        const int slot = t.commit[3 * j], tl = t.commit[3 * j + 1];
        if (slot < 0 || slot >= t.S || tl < 0 || tl > t.max_trailing) { *t.error = 1; continue; }
        t.trailing_len[slot] = tl;
        t.n_tokens[slot] = t.commit[3 * j + 2];
    }
}
bool text_append(const TextAppend &t, hipStream_t s) {
    if (t.n_rows < 0 || t.n_commit < 0 || t.H <= 0 || t.H % 4 != 0 || t.S <= 0 || t.max_trailing <= 0 || !t.error ||
        (t.n_rows > 0 && !(t.src && t.trailing && t.rows)) || (t.n_commit > 0 && !(t.commit && t.trailing_len && t.n_tokens))) {
        set_error("text_append: bad parameters");
        return false;
    }
    if (t.n_rows + t.n_commit == 0) return true;
    hipLaunchKernelGGL(k_text_append, dim3((unsigned)t.n_rows + 1), dim3(256), 0, s, t);
    Q3T_HIP(hipGetLastError());
    return true;
}

// every thread reads the slot's flags before thread 0 rewrites them (the barrier)
template <bool HOLD>
__global__ void __launch_bounds__(256) k_slot_hold(const SlotHold h) {
    const int k = blockIdx.x;
    if (!h.mask[k]) return;
    const int done = h.done[k], held = h.held[k], frame = h.frame[k];
    __syncthreads();
    if (HOLD ? done >= 0 : !held) return;   // uniform over the workgroup
    const float4 *from = reinterpret_cast<const float4 *>((HOLD ? h.hidden : h.save) + (size_t)k * h.H);
    float4 *to = reinterpret_cast<float4 *>((HOLD ? h.save : h.hidden) + (size_t)k * h.H);
    for (int i = threadIdx.x; i < h.H / 4; i += 256) to[i] = from[i];
    if (threadIdx.x == 0) {
        h.done[k] = HOLD ? frame : -1;
        h.held[k] = HOLD ? 1 : 0;
    }
}
static bool slot_hold_args(const SlotHold &h) {
    if (h.H <= 0 || h.H % 4 != 0 || !h.mask || !h.hidden || !h.save || !h.done || !h.held || !h.frame) {
        set_error("slot_hold: bad parameters");
        return false;
    }
    return true;
}
bool slot_hold(const SlotHold &h, int S, hipStream_t s) {
    if (!slot_hold_args(h)) return false;
    if (S <= 0) return true;
    hipLaunchKernelGGL(k_slot_hold<true>, dim3(S), dim3(256), 0, s, h);
    Q3T_HIP(hipGetLastError());
    return true;
}
bool slot_release(const SlotHold &h, int S, hipStream_t s) {
    if (!slot_hold_args(h)) return false;
    if (S <= 0) return true;
    hipLaunchKernelGGL(k_slot_hold<false>, dim3(S), dim3(256), 0, s, h);
    Q3T_HIP(hipGetLastError());
    return true;
}

__global__ void k_rows_recipe(const RowRecipe *rec, int H) {
    const RowRecipe R = rec[blockIdx.x];
    for (int h = threadIdx.x; h < H; h += blockDim.x) {
        float v = 0.0f;
        bool first = true;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            if (!R.t[t].ptr) continue;
            const float x = R.t[t].is_f16 ? h2f(reinterpret_cast<const uint16_t *>(R.t[t].ptr)[h])
                                          : reinterpret_cast<const float *>(R.t[t].ptr)[h];
            v = first ? x : v + x;
            first = false;
        }
        R.out[h] = v;
    }
}
bool rows_recipe(const RowRecipe *recipe_dev, int n_rows, int H, hipStream_t s) {
    if (n_rows <= 0) return true;
    hipLaunchKernelGGL(k_rows_recipe, dim3(n_rows), dim3(256), 0, s, recipe_dev, H);
    Q3T_HIP(hipGetLastError());
    return true;
}


// ---------------------------------------------------------------- trt_cuda_kernels.cu drop-ins
__global__ void k_f32_to_f16(const float *in, uint16_t *out, int n) {
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        const float4 v = *reinterpret_cast<const float4 *>(in + i);
        out[i] = f2h(v.x); out[i + 1] = f2h(v.y); out[i + 2] = f2h(v.z); out[i + 3] = f2h(v.w);
    } else {
        for (int j = i; j < n; ++j) out[j] = f2h(in[j]);
    }
}
__global__ void __launch_bounds__(256) k_argmax_f32(const float *in, int32_t *out, int n) {
    __shared__ SelLds S;
    if (n <= 256 * SEL_VPT_MAX) {
        float v[SEL_VPT_MAX];
        const int vpt = (n + 255) / 256;
        sel_load<false>(in, n, vpt, v);
        const int r = sel_argmax(v, n, vpt, S);
        if (threadIdx.x == 0) *out = r;
        return;
    }
    // any n (the reference wrapper accepts any length): strided scan, lowest index wins ties
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 256)
        if (in[i] > bv || bi == 0x7fffffff) { bv = in[i]; bi = i; }
    sel_pair_reduce(bv, bi);
    if ((threadIdx.x & 63) == 0) { S.fred[threadIdx.x >> 6] = bv; S.ired[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (S.fred[w] > S.fred[0] || (S.fred[w] == S.fred[0] && S.ired[w] < S.ired[0])) { S.fred[0] = S.fred[w]; S.ired[0] = S.ired[w]; }
        *out = S.ired[0] == 0x7fffffff ? 0 : S.ired[0];
    }
}
__global__ void k_embed_lookup(const int32_t *tok, const float *table, float *out, int dim) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < dim) out[i] = table[(size_t)(*tok) * dim + i];
}
__global__ void __launch_bounds__(256) k_sample_topk_f32(const float *logits, const float *rand_val, int32_t *out,
                                                          float temperature, int top_k, int n) {
    __shared__ SelLds S;
    float v[SEL_VPT_MAX];
    const int vpt = (n + 255) / 256;
    sel_load<false>(logits, n, vpt, v);
    const int r = temperature <= 0.0f ? sel_argmax(v, n, vpt, S) : sel_sample(v, n, vpt, temperature, top_k, *rand_val, -1, S);
    if (threadIdx.x == 0) *out = r;
}
void launch_f32_to_f16(const float *in, uint16_t *out, int n, hipStream_t s) {
    hipLaunchKernelGGL(k_f32_to_f16, dim3((n + 1023) / 1024), dim3(256), 0, s, in, out, n);
}
void launch_argmax_f32(const float *in, int32_t *out, int n, hipStream_t s) {
    hipLaunchKernelGGL(k_argmax_f32, dim3(1), dim3(256), 0, s, in, out, n);
}
void launch_embed_lookup(const int32_t *tok, const float *table, float *out, int dim, hipStream_t s) {
    hipLaunchKernelGGL(k_embed_lookup, dim3((dim + 255) / 256), dim3(256), 0, s, tok, table, out, dim);
}
void launch_sample_topk_f32(const float *logits, const float *rand_val, int32_t *out, float temperature, int top_k, int n,
                            hipStream_t s) {
    hipLaunchKernelGGL(k_sample_topk_f32, dim3(1), dim3(256), 0, s, logits, rand_val, out, temperature, top_k, n);
}

// ------------------------------------------------------------------------------------------ batched residual + norm
// one workgroup per token; thread t owns elements 4t .. 4t+3 of every 1024-wide chunk of the row: W = 1 chunk for
// H <= 1024 (the 0.6B widths and both code predictors), W = 2 for the 1.7B talker's 2,048 -- the narrow form's
// arithmetic is that of W = 1 term for term, so its bits do not depend on the wide form existing.  Partial slabs are
// added in slice order; the RMS sum runs in double over the block (gemv.hip / gemm_mfma.hip prologue numerics), a
// thread's chunks in ascending order before the wave reduction.  KS (the slab count) is a template argument so the x
// and slab loads issue back to back: with a runtime count each sat in its own branch and waited for its own round
// trip.
// Workgroups past the S token rows only prefetch (ResidNorm::prefetch): global->LDS dword loads, one per 128-B line
// of the next projection's weights, which leave no register to wait on; the lines land in the Infinity Cache.
constexpr int RN_PF_LINES = 2;   // prefetched lines per thread
template <int KS, int W>
__global__ void __launch_bounds__(256) k_resid_norm(const ResidNorm r) {
    __shared__ double scr[4];
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= r.S) {
        __shared__ uint32_t sink[256];
        const size_t lines = r.prefetch_bytes / 128, nthr = (size_t)(gridDim.x - r.S) * 256;
#pragma unroll
        for (int q = 0; q < RN_PF_LINES; ++q) {
            const size_t line = (size_t)q * nthr + (size_t)(b - r.S) * 256 + t;
            if (line < lines)
                __builtin_amdgcn_global_load_lds(static_cast<const uint8_t *>(r.prefetch) + line * 128,
                                                 (__attribute__((address_space(3))) void *)sink, 4, 0, 0);
        }
        return;
    }
    bool ok[W];
    size_t o[W];
    float4 x[W], pz[W][KS > 0 ? KS : 1];
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const int k = 4 * t + 1024 * i;
        ok[i] = k < r.H;
        o[i] = (size_t)b * r.H + (ok[i] ? k : 0);
        x[i] = *reinterpret_cast<const float4 *>((r.xin ? r.xin : r.x) + o[i]);
    }
#pragma unroll
    for (int i = 0; i < W; ++i)
#pragma unroll
        for (int z = 0; z < KS; ++z) pz[i][z] = *reinterpret_cast<const float4 *>(r.parts + (size_t)z * r.S * r.H + o[i]);
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        float4 v = x[i];
#pragma unroll
        for (int z = 0; z < KS; ++z) v = make_float4(v.x + pz[i][z].x, v.y + pz[i][z].y, v.z + pz[i][z].z, v.w + pz[i][z].w);
        if (!ok[i]) v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[i] && (KS > 0 || (r.xin && r.xin != r.x))) *reinterpret_cast<float4 *>(r.x + o[i]) = v;
        const double si = (double)(v.x * v.x) + (double)(v.y * v.y) + (double)(v.z * v.z) + (double)(v.w * v.w);
        ss = i == 0 ? si : ss + si;
        x[i] = v;
    }
    ss = wave_sum_d(ss);
    if ((t & 63) == 0) scr[t >> 6] = ss;
    __syncthreads();
    ss = (scr[0] + scr[1]) + (scr[2] + scr[3]);
    const float scale = 1.0f / sqrtf((float)(ss / r.H) + r.eps);
#pragma unroll
    for (int i = 0; i < W; ++i) {
        if (!ok[i]) continue;
        const float4 v = x[i];
        const float4 w = *reinterpret_cast<const float4 *>(r.nw + 4 * t + 1024 * i);
        const float y0 = (v.x * scale) * w.x, y1 = (v.y * scale) * w.y, y2 = (v.z * scale) * w.z, y3 = (v.w * scale) * w.w;
        if (r.side) *reinterpret_cast<float4 *>(r.side + o[i]) = make_float4(y0, y1, y2, y3);
        uint2 h;
        h.x = (uint32_t)f2h(y0) | ((uint32_t)f2h(y1) << 16);
        h.y = (uint32_t)f2h(y2) | ((uint32_t)f2h(y3) << 16);
        *reinterpret_cast<uint2 *>(r.xn + o[i]) = h;
    }
}
// W as k_resid_norm's.  F32TAB: the nt = 1 source is an f32 row of EmbedNorm::ftab (the 1.7B code predictor's
// projected pass inputs) instead of an f16 table row.
template <int W, bool F32TAB, bool REC>
__global__ void __launch_bounds__(256) k_select_embed_norm(const SelectSpec sp, const float *logits, const EmbedNorm en) {
    __shared__ SelLds S;
    __shared__ double scr[4];
    __shared__ int stok;
    const int b = blockIdx.x, t = threadIdx.x;
    const int tok = select_token<false, REC>(sp, logits + (size_t)b * sp.V, b, S);
    if (t == 0) {
        if (tok >= 0) select_commit(sp, b, tok);
        stok = tok;
    }
    __syncthreads();
    const int sel_col = sp.mode == SEL_CB0 ? 0 : sp.step + 1;   // the column this launch selected
    const GatherSum &gs = en.gs;
    auto token = [&](int col) {   // finished slots (no selection) keep the token already in the table
        const int tt = gs.tok[(size_t)b * gs.tok_ld + col];   // loaded unconditionally: no branch around the load
        return col == sel_col && stok >= 0 ? stok : tt;
    };
    bool ok[W];
    int kk[W];
    float a[W][4];
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const int k = 4 * t + 1024 * i;
        ok[i] = k < en.H;
        kk[i] = ok[i] ? k : 0;
    }
    if constexpr (F32TAB) {
        const float *r0 = en.ftab + (en.ftab_row0 + (size_t)token(gs.tok_col0)) * en.H;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const float4 e = *reinterpret_cast<const float4 *>(r0 + kk[i]);
            a[i][0] = e.x; a[i][1] = e.y; a[i][2] = e.z; a[i][3] = e.w;
        }
    } else {
        {
            const uint16_t *r0 = en.nt == 1 ? gs.tab0 + (size_t)token(gs.tok_col0) * en.H : gs.tabs[0] + (size_t)token(0) * en.H;
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const uint2 u = *reinterpret_cast<const uint2 *>(r0 + kk[i]);
                a[i][0] = h2f(u.x & 0xffff); a[i][1] = h2f(u.x >> 16); a[i][2] = h2f(u.y & 0xffff); a[i][3] = h2f(u.y >> 16);
            }
        }
        if (en.nt == 16) {
#pragma unroll   // the 15 token loads, then the 15 row loads, each group in flight together
            for (int j = 1; j < 16; ++j) {
                const uint16_t *rj = gs.tabs[j] + (size_t)token(j) * en.H;
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const uint2 u = *reinterpret_cast<const uint2 *>(rj + kk[i]);
                    a[i][0] += h2f(u.x & 0xffff); a[i][1] += h2f(u.x >> 16); a[i][2] += h2f(u.y & 0xffff); a[i][3] += h2f(u.y >> 16);
                }
            }
            const int fr = gs.frame[b];
            const float *extra = fr < gs.tr_len[b] ? gs.tr + (size_t)b * gs.tr_ld + (size_t)fr * en.H : gs.pad + (size_t)b * en.H;
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const float4 e = *reinterpret_cast<const float4 *>(extra + kk[i]);
                a[i][0] += e.x; a[i][1] += e.y; a[i][2] += e.z; a[i][3] += e.w;
            }
        }
    }
    float4 x[W];
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        x[i] = ok[i] ? make_float4(a[i][0], a[i][1], a[i][2], a[i][3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[i]) *reinterpret_cast<float4 *>(en.x + (size_t)b * en.H + kk[i]) = x[i];
        const float4 v = x[i];
        const double si = (double)(v.x * v.x) + (double)(v.y * v.y) + (double)(v.z * v.z) + (double)(v.w * v.w);
        ss = i == 0 ? si : ss + si;
    }
    ss = wave_sum_d(ss);
    if ((t & 63) == 0) scr[t >> 6] = ss;
    __syncthreads();
    ss = (scr[0] + scr[1]) + (scr[2] + scr[3]);
    const float scale = 1.0f / sqrtf((float)(ss / en.H) + en.eps);
#pragma unroll
    for (int i = 0; i < W; ++i) {
        if (!ok[i]) continue;
        const float4 v = x[i];
        const float4 w = *reinterpret_cast<const float4 *>(en.nw + 4 * t + 1024 * i);
        const float y0 = (v.x * scale) * w.x, y1 = (v.y * scale) * w.y, y2 = (v.z * scale) * w.z, y3 = (v.w * scale) * w.w;
        uint2 h;
        h.x = (uint32_t)f2h(y0) | ((uint32_t)f2h(y1) << 16);
        h.y = (uint32_t)f2h(y2) | ((uint32_t)f2h(y3) << 16);
        *reinterpret_cast<uint2 *>(en.xn + (size_t)b * en.H + kk[i]) = h;
    }
}
bool select_embed_norm(const SelectSpec &sp, const float *logits, const EmbedNorm &en, int S, hipStream_t s) {
    if (sp.V > 256 * SEL_VPT_MAX || sp.V <= 0) { set_error("select: vocab must be in (0, 4096]"); return false; }
    const bool f32tab = en.ftab != nullptr;
    if (en.H > (f32tab ? 1024 : 2048) || en.H % 4 != 0 || !en.x || !en.xn || !en.nw || (en.nt != 1 && en.nt != 16) ||
        (en.nt == 1 && !en.gs.tab0 && !f32tab) || (f32tab && en.nt != 1) ||
        (en.nt == 16 && !(en.gs.tabs && en.gs.frame && en.gs.tr_len && en.gs.pad)) || !en.gs.tok) {
        set_error("select_embed_norm: bad parameters");
        return false;
    }
    if (S <= 0) return true;
#define Q3T_SEN_LAUNCH(WW, FF)                                                                                       \
    do {                                                                                                            \
        if (sp.rec) hipLaunchKernelGGL((k_select_embed_norm<WW, FF, true>), dim3(S), dim3(256), 0, s, sp, logits, en);   \
        else hipLaunchKernelGGL((k_select_embed_norm<WW, FF, false>), dim3(S), dim3(256), 0, s, sp, logits, en);         \
    } while (0)
    if (f32tab) Q3T_SEN_LAUNCH(1, true);
    else if (en.H > 1024) Q3T_SEN_LAUNCH(2, false);
    else Q3T_SEN_LAUNCH(1, false);
#undef Q3T_SEN_LAUNCH
    Q3T_HIP(hipGetLastError());
    return true;
}

// out[b] = tab[row0 + tok[b * tok_ld + col]] (f32 rows of H): pass 1 of the 1.7B code predictor on the matrix-core
// stack, whose CB0 was selected by the talker's launch (every later pass's row comes with its selection hand-off)
__global__ void __launch_bounds__(256) k_gather_rows_f32(const float *tab, size_t row0, const int *tok, int tok_ld, int col,
                                                         int H, float *out) {
    const int b = blockIdx.x;
    const float *row = tab + (row0 + (size_t)tok[(size_t)b * tok_ld + col]) * H;
    for (int k = threadIdx.x * 4; k < H; k += 1024)
        *reinterpret_cast<float4 *>(out + (size_t)b * H + k) = *reinterpret_cast<const float4 *>(row + k);
}
bool gather_rows_f32(const float *tab, size_t row0, const int *tok, int tok_ld, int col, int S, int H, float *out, hipStream_t s) {
    if (H % 4 != 0 || !tab || !tok || !out) { set_error("gather_rows_f32: bad parameters"); return false; }
    if (S <= 0) return true;
    hipLaunchKernelGGL(k_gather_rows_f32, dim3(S), dim3(256), 0, s, tab, row0, tok, tok_ld, col, H, out);
    Q3T_HIP(hipGetLastError());
    return true;
}

int resid_norm_chunks(int H) { return H <= 1024 ? 1 : 2; }
template <int W>
static void launch_resid_norm(const ResidNorm &r, dim3 grid, hipStream_t s) {
    switch (r.parts ? r.ksplit : 0) {
        case 0: hipLaunchKernelGGL((k_resid_norm<0, W>), grid, dim3(256), 0, s, r); break;
        case 1: hipLaunchKernelGGL((k_resid_norm<1, W>), grid, dim3(256), 0, s, r); break;
        case 2: hipLaunchKernelGGL((k_resid_norm<2, W>), grid, dim3(256), 0, s, r); break;
        case 3: hipLaunchKernelGGL((k_resid_norm<3, W>), grid, dim3(256), 0, s, r); break;
        default: hipLaunchKernelGGL((k_resid_norm<4, W>), grid, dim3(256), 0, s, r); break;
    }
}
bool resid_norm(const ResidNorm &r, hipStream_t s) {
    if (r.S <= 0) return true;
    if (r.H > 2048 || r.H % 4 != 0 || !r.x || !r.nw || !r.xn || (r.parts && (r.ksplit < 1 || r.ksplit > 4))) {
        set_error("resid_norm: unsupported shape");
        return false;
    }
    const size_t pf_lines = r.prefetch ? r.prefetch_bytes / 128 : 0;
    const unsigned pf_wgs = (unsigned)std::min<size_t>((pf_lines + 256 * RN_PF_LINES - 1) / (256 * RN_PF_LINES), 1024);
    const dim3 grid((unsigned)r.S + pf_wgs);
    if (resid_norm_chunks(r.H) == 1) launch_resid_norm<1>(r, grid, s);
    else launch_resid_norm<2>(r, grid, s);
    Q3T_HIP(hipGetLastError());
    return true;
}

}  // namespace q3t
