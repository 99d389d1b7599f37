// pcm_out.hip — the output stage's filter design (host) and its two kernels (see pcm_out.h, DESIGN 2c "Output stage").
#include "pcm_out.h"

#include <atomic>
#include <cmath>
#include <numeric>
#include <string>

#include "q3t_common.h"

namespace q3t {

namespace {
constexpr int kRates[] = {8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000};
constexpr int kWinFloats = 3 * kPcmBlockOut + 128;   // M / L <= 3 and K <= 97 over the supported rates
std::atomic<int64_t> g_launches{0};

// I0 by its power series, in double: sum ((x/2)^k / k!)^2
double bessel_i0(double x) {
    const double q = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}
}  // namespace

const char *pcm_rates_text() { return "8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000"; }

bool pcm_rate(int rate, PcmRate *out) {
    bool known = false;
    for (int r : kRates) known = known || r == rate;
    if (!known) return false;
    PcmRate g;
    if (rate != kPcmNativeRate) {
        const int gc = std::gcd(rate, kPcmNativeRate);
        g.L = rate / gc;
        g.M = kPcmNativeRate / gc;
        const int R = std::max(g.L, g.M), N = 2 * kPcmZ * R + 1;
        g.K = (N + g.L - 1) / g.L;
        g.D = (kPcmZ * R + g.L - 1) / g.L;
    }
    if (out) *out = g;
    return true;
}

int pcm_bytes_per_sample(int format) { return format == kPcmF32 ? 4 : format == kPcmS16 ? 2 : format == kPcmMulaw ? 1 : 0; }

int64_t pcm_num_samples(int64_t n_in_total, int rate, bool final) {
    PcmRate g;
    if (!pcm_rate(rate, &g) || n_in_total < 0) return -1;
    const int64_t S = n_in_total + (final ? g.D : 0);
    return (S * g.L + g.M - 1) / g.M;
}

bool pcm_taps(int rate, PcmRate *geo, std::vector<float> *taps) {
    PcmRate g;
    if (!pcm_rate(rate, &g)) return false;
    if (geo) *geo = g;
    if (!taps) return true;
    taps->assign((size_t)g.L * g.K, 0.0f);
    if (g.K == 0) return true;
    const int R = std::max(g.L, g.M), N = 2 * kPcmZ * R + 1, c = kPcmZ * R;
    const double f = 0.9 / (double)R, beta = 9.0, pi = 3.14159265358979323846, i0b = bessel_i0(beta);
    for (int p = 0; p < g.L; ++p)
        for (int k = 0; k < g.K; ++k) {
            const int j = p + k * g.L;
            if (j >= N) continue;
            const double u = (double)(j - c), x = f * u, r = u / (double)c;
            const double sinc = j == c ? 1.0 : std::sin(pi * x) / (pi * x);
            const double w = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
            (*taps)[(size_t)p * g.K + k] = (float)((double)g.L * (f * sinc * w));
        }
    return true;
}

// ------------------------------------------------------------------------------------------------------- kernels
namespace {

// save_audio_file's rule: clamp, scale by 32767, truncate toward zero.  For finite samples the value is the host
// loop's; a NaN (whose host cast is undefined) is dropped by fmaxf / fminf and comes out as -32767
__device__ __forceinline__ int to_s16(float y) {
    const float c = fminf(fmaxf(y, -1.0f), 1.0f) * 32767.0f;
    return (int)c;
}
// G.711 mu-law of an s16 value: bias 0x84, clip 32635, sign / exponent / mantissa complemented
__device__ __forceinline__ unsigned to_mulaw(int v) {
    const unsigned sign = v < 0 ? 0x80u : 0u;
    int m = v < 0 ? -v : v;
    m = (m > 32635 ? 32635 : m) + 132;               // 132 .. 32767: the top set bit is bit 7 .. 14
    const int e = 24 - __clz(m);                     // 0 .. 7
    const unsigned mant = ((unsigned)m >> (e + 3)) & 0xFu;
    return ~(sign | ((unsigned)e << 4) | mant) & 0xFFu;
}

// A workgroup takes kPcmBlockOut consecutive outputs of one stream (blockIdx.y), counted from the 4-sample group
// boundary at or below the stream's output pointer, so that every full group of four is one aligned vector store.
__global__ void __launch_bounds__(256) k_pcm_out(const PcmOutDesc *descs) {
    __shared__ float win[kWinFloats];
    const PcmOutDesc d = descs[blockIdx.y];
    const int bps = d.format == kPcmF32 ? 4 : d.format == kPcmS16 ? 2 : 1;
    const int mis = (int)(((uintptr_t)d.out % (uintptr_t)(4 * bps)) / (uintptr_t)bps);   // samples past the group boundary
    const int64_t v0 = (int64_t)blockIdx.x * kPcmBlockOut - mis;   // output index of this workgroup's first lane slot
    const int o_lo = (int)(v0 < 0 ? 0 : v0);
    const int o_hi = (int)(v0 + kPcmBlockOut < (int64_t)d.n_out ? v0 + kPcmBlockOut : (int64_t)d.n_out);
    if (o_lo >= o_hi) return;   // uniform over the workgroup
    const int H = d.K - 1;
    int lo = 0;   // first input sample of the window, relative to x[0] (>= -H)
    if (d.K > 0) {
        lo = (int)(((d.n0 + o_lo) * d.M) / d.L - d.s0) - H;
        const int hi = (int)(((d.n0 + o_hi - 1) * d.M) / d.L - d.s0);
        const int W = hi - lo + 1;   // <= (kPcmBlockOut - 1) * M / L + 1 + K <= kWinFloats
        for (int w = threadIdx.x; w < W; w += blockDim.x) {
            const int li = lo + w;
            win[w] = li < 0 ? d.hist[H + li] : li < d.n_in ? d.x[li] : 0.0f;
        }
        __syncthreads();
    }
    float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int64_t vb = v0 + 4 * (int)threadIdx.x;
    bool ok[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t o = vb + e;
        ok[e] = o >= o_lo && o < o_hi;
        if (!ok[e]) continue;
        if (d.K == 0) { y[e] = d.x[o]; continue; }   // native rate: the input, bit for bit
        const int64_t t = (d.n0 + o) * d.M;
        const int i = (int)(t / d.L - d.s0) - lo, p = (int)(t % d.L);
        const float *tp = d.taps + (size_t)p * d.K;
        float acc = 0.0f;
        for (int k = 0; k < d.K; ++k) acc = fmaf(tp[k], win[i - k], acc);   // the pinned order: k upward from 0.0f
        y[e] = acc;
    }
    const bool full = ok[0] && ok[1] && ok[2] && ok[3];
    if (d.format == kPcmF32) {
        float *o = static_cast<float *>(d.out) + vb;
        if (full) *reinterpret_cast<float4 *>(o) = make_float4(y[0], y[1], y[2], y[3]);
        else
#pragma unroll
            for (int e = 0; e < 4; ++e) if (ok[e]) o[e] = y[e];
    } else if (d.format == kPcmS16) {
        int16_t *o = static_cast<int16_t *>(d.out) + vb;
        int v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = to_s16(y[e]);
        if (full)
            *reinterpret_cast<uint2 *>(o) = make_uint2(((unsigned)v[0] & 0xFFFFu) | ((unsigned)v[1] << 16),
                                                       ((unsigned)v[2] & 0xFFFFu) | ((unsigned)v[3] << 16));
        else
#pragma unroll
            for (int e = 0; e < 4; ++e) if (ok[e]) o[e] = (int16_t)v[e];
    } else {
        uint8_t *o = static_cast<uint8_t *>(d.out) + vb;
        unsigned v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = to_mulaw(to_s16(y[e]));
        if (full) *reinterpret_cast<uint32_t *>(o) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        else
#pragma unroll
            for (int e = 0; e < 4; ++e) if (ok[e]) o[e] = (uint8_t)v[e];
    }
}

// the next push's history: the last K - 1 samples of [hist | x | n_zero zeros], one workgroup per stream
__global__ void __launch_bounds__(128) k_pcm_out_hist(const PcmOutDesc *descs) {
    const PcmOutDesc d = descs[blockIdx.x];
    const int H = d.K - 1, t = threadIdx.x;
    float v = 0.0f;
    if (t < H) {
        const int64_t src = (int64_t)d.n_in + d.n_zero + t;   // index into the concatenation, whose first H are hist
        v = src < H ? d.hist[src] : src - H < d.n_in ? d.x[src - H] : 0.0f;
    }
    __syncthreads();   // every read of hist before any write of it
    if (t < H) d.hist[t] = v;
}

}  // namespace

bool pcm_out(const PcmOutDesc *descs, int n_streams, int64_t max_out, hipStream_t s) {
    if (n_streams <= 0) { set_error("pcm_out: n_streams must be > 0"); return false; }
    if (!descs) { set_error("pcm_out: null descriptors"); return false; }
    if (max_out < 0 || max_out > ((int64_t)1 << 31) - 2 * kPcmBlockOut) { set_error("pcm_out: output count out of range"); return false; }
    if (n_streams > 65535) { set_error("pcm_out: more than 65535 streams in one launch"); return false; }
    // + 3: a stream whose pointer sits past a group boundary starts up to 3 lane slots into its first workgroup
    const unsigned gx = (unsigned)std::max<int64_t>((max_out + 3 + kPcmBlockOut - 1) / kPcmBlockOut, 1);
    hipLaunchKernelGGL(k_pcm_out, dim3(gx, (unsigned)n_streams), dim3(256), 0, s, descs);
    Q3T_HIP(hipGetLastError());
    ++g_launches;
    return true;
}

bool pcm_out_hist(const PcmOutDesc *descs, int n_streams, hipStream_t s) {
    if (n_streams <= 0) { set_error("pcm_out_hist: n_streams must be > 0"); return false; }
    if (!descs) { set_error("pcm_out_hist: null descriptors"); return false; }
    static_assert(kPcmMaxHist <= 128, "k_pcm_out_hist covers the history with one 128-thread workgroup");
    hipLaunchKernelGGL(k_pcm_out_hist, dim3((unsigned)n_streams), dim3(128), 0, s, descs);
    Q3T_HIP(hipGetLastError());
    return true;
}

int64_t pcm_out_launches() { return g_launches.load(); }

}  // namespace q3t
