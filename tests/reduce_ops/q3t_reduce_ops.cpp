// q3t_reduce_ops.cpp — test-only C entry point over the wave reduction helpers of csrc/q3t_common.h that the one-slot
// role kernels' bodies are built from (tests/test_gpu_reduce_ops.py): one launch runs, per 64-lane vector,
//   group_sum<16> of four neighbouring accumulators (the role bodies' pattern: DPP row steps),
//   wave_sum_d (DPP steps that leave their destination uninitialised, then the row swaps),
//   the QKV publish's reduce-scatter + row gather (group16_sum_scatter4, rows_gather16, scatter4_index)
// beside the forms they replaced or must equal, written out here with no DPP fold to lose: the same trees over
// __shfl (ds_bpermute), update_dpp with a zero old value, and the publish through four __shfl of four group sums.
// Like tests/attn_ops/ this is a library of its own, built with csrc's compiler and the role kernels' flags; it needs
// no launcher of libq3t.so, only the header.  Returns 0, or -1 with the error text in err.
#include <cstdint>
#include <cstring>
#include <string>

#include "q3t_common.h"

using namespace q3t;

namespace {

// lane ^ 1, lane ^ 2, row_half_mirror, row_mirror as generic shuffles
__device__ float shfl_step(float v, int step) {
    const int l = threadIdx.x & 63;
    const int src = step == 0 ? l ^ 1 : step == 1 ? l ^ 2 : step == 2 ? (l & ~7) | (7 - (l & 7)) : (l & ~15) | (15 - (l & 15));
    return __shfl(v, src);
}
__device__ float group_sum16_shfl(float v) {
    for (int s = 0; s < 4; ++s) v += shfl_step(v, s);
    return v;
}
template <int CTRL>
__device__ double dpp_d_zero_old(double v) {   // the earlier dpp_d: old = 0, no bound_ctrl
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const unsigned lo = dpp_u<CTRL>((unsigned)u), hi = dpp_u<CTRL>((unsigned)(u >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ double wave_sum_d_zero_old(double v) {
    v += dpp_d_zero_old<DPP_XOR1>(v);
    v += dpp_d_zero_old<DPP_XOR2>(v);
    v += dpp_d_zero_old<DPP_HALF_MIRROR>(v);
    v += dpp_d_zero_old<DPP_MIRROR>(v);
    v += xrow16_d(v);
    v += xrow32_d(v);
    return v;
}

// block v: vector v.  in_f [nv][4][64], in_d [nv][64]; gs_* [nv][4][64], ws_* [nv][64], pub_* [nv][16] (row 4j + g: the
// sum of accumulator j over the 16-lane group g)
__global__ void __launch_bounds__(64) k_reduce_forms(const float *in_f, const double *in_d, float *gs_new, float *gs_ref,
                                                     double *ws_new, double *ws_ref, float *pub_new, float *pub_ref) {
#pragma clang fp contract(off)
    const int v = blockIdx.x, lane = threadIdx.x;
    float acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = in_f[((size_t)v * 4 + j) * 64 + lane];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        gs_new[((size_t)v * 4 + j) * 64 + lane] = group_sum<16>(acc[j]);
        gs_ref[((size_t)v * 4 + j) * 64 + lane] = group_sum16_shfl(acc[j]);
    }
    const double d = in_d[(size_t)v * 64 + lane];
    ws_new[(size_t)v * 64 + lane] = wave_sum_d(d);
    ws_ref[(size_t)v * 64 + lane] = wave_sum_d_zero_old(d);
    {   // the publish as persist_roles.h's qkv_phase does it
        const float pv = rows_gather16(group16_sum_scatter4(acc));
        if (lane < 16) pub_new[(size_t)v * 16 + 4 * scatter4_index(lane) + (lane >> 2)] = pv;
    }
    {   // and as it did: lane L < 16 takes row 4j + g (j = L / 4, g = L % 4) from lane 16 g
        float pv = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = __shfl(group_sum16_shfl(acc[j]), 16 * (lane & 3));
            if ((lane >> 2) == j) pv = s;
        }
        if (lane < 16) pub_ref[(size_t)v * 16 + lane] = pv;
    }
}

template <typename T> T *ptr(uint64_t v) { return reinterpret_cast<T *>(static_cast<uintptr_t>(v)); }

}  // namespace

extern "C" int q3t_ops_reduce_forms(uint64_t in_f, uint64_t in_d, int nv, uint64_t gs_new, uint64_t gs_ref, uint64_t ws_new,
                                    uint64_t ws_ref, uint64_t pub_new, uint64_t pub_ref, char *err, int errlen) {
    std::string msg;
    if (nv <= 0 || !in_f || !in_d || !gs_new || !gs_ref || !ws_new || !ws_ref || !pub_new || !pub_ref) {
        msg = "q3t_ops_reduce_forms: bad parameters";
    } else {
        hipLaunchKernelGGL(k_reduce_forms, dim3(nv), dim3(64), 0, nullptr, ptr<const float>(in_f), ptr<const double>(in_d),
                           ptr<float>(gs_new), ptr<float>(gs_ref), ptr<double>(ws_new), ptr<double>(ws_ref), ptr<float>(pub_new),
                           ptr<float>(pub_ref));
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) return 0;
        msg = std::string("k_reduce_forms: ") + hipGetErrorString(e);
    }
    if (err && errlen > 0) {
        std::strncpy(err, msg.c_str(), (size_t)errlen - 1);
        err[errlen - 1] = 0;
    }
    return -1;
}
