// Non-parallel evaluation: modulation spectra, global variance and the distance between two SETS of utterances (definitions:
// mask_cyclegan_vc/metrics.py).  No alignment, no atomics; every reduction runs in an order that depends on the utterance alone.
//
//   ms_power_kernel<MT>   one launch for a whole ragged cepstra bank [K][N].  A workgroup of four waves owns one utterance and 128
//                         consecutive bins; a wave owns 32 bins f (the lanes of an accumulator run along f: coalesced stores of P[u][k][f])
//                         and MT row tiles of 32 cepstral rows, with separate re and im accumulators: a matrix product
//                         [K, T] x [T, 2 x 32] on v_mfma_f32_32x32x2_f32 whose B operand is never stored.  Each lane forms it from the cosine
//                         table in LDS (<= 16 KB) at the INTEGER phase (f t) mod n_fft, advanced by 2 f per MFMA step and masked; the
//                         sine is the same table a quarter turn on (cos(a + pi/2) = -sin a, the imaginary part of exp(-i a)).
//                         Pre-pass, per row, lane l summing t = l, l + 64, .. and a fixed butterfly over the lanes:
//                           m0 = (sum c) / T,  r = (sum (c - m0)) / T,  x[t] = (c[t] - m0) - r,  mean = m0 + r,  var = (sum x^2) / T.
//                         The correction r keeps the error of x in terms of sum |x| rather than sum |c| (m0 alone is only as good as
//                         |mean| 2^-24), and makes a constant row come out as x == 0 exactly.  Every workgroup of an utterance computes
//                         the same m0 and r; the workgroup of bin group 0 writes mean and var.
//                         The trajectory is staged in LDS in chunks of 64 frames, mean-subtracted, zero at t >= T and rows >= K, frame tt of
//                         row k at 97 tt + k: the A reads (32 lanes along k) and the staging writes (32 lanes along tt) are both free of
//                         bank conflicts.  Two levels of accumulation, as stft_product's FLUSH_KG: a chunk is summed from zero (a chain
//                         of at most 64) and then added to the running total (at most 64 additions for T = 4096), so no chain is T long.
//                         Epilogue: P = (re^2 + im^2) / T.  Only [offs[u], offs[u + 1]) of a row is ever read.
//   ms_mean_log_kernel    out[r] = (1 / n) sum_u 10 log10(max(v[u][r], floor)), utterances in index order; one thread per r.
//   ms_distance_kernel    one workgroup: per row k the squared differences of the first F bins (lane l: f = l, l + 64, ..; butterfly), then
//                         the rows in the same way; per_dim[k] = sqrt(S_k / F), total = sqrt(sum_k S_k / (K F)).
#include <cmath>
#include <cstdint>

#include "mcvc_common.h"
#include "ms.h"
#include "trace.h"

namespace {

constexpr int MAXFFT = MCVC_MS_MAX_FFT, MAXK = MCVC_MS_MAX_K;
constexpr int NTHREADS = 256, WAVES = NTHREADS / 64;
constexpr int BINS_PER_WG = 32 * WAVES;                  // 128
constexpr int TC = 64;                                   // frames per staged chunk (the inner chain)
constexpr int PITCH = 97;                                // floats from one staged frame to the next: odd, >= 96 rows
constexpr double kPi = 3.14159265358979323846;
static_assert((MCVC_MS_MIN_FFT / 2) % BINS_PER_WG == 0, "whole bin groups");
static_assert(PITCH >= 32 * 3 && (PITCH & 1), "three row tiles, conflict-free staging");

struct MsArgs {
    const float* cep; const int* offs; const float* table;
    float* power; float* mean; float* var;
    long long n_frames;
    int K, n_utts, n_fft;
};

// the sum of the lanes' values in a fixed order (the same bits in every lane: a + b == b + a)
__device__ __forceinline__ float wave_sum(float s)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s = __fadd_rn(s, __shfl_xor(s, m));
    return s;
}

template <int MT>
__global__ __launch_bounds__(NTHREADS) void ms_power_kernel(MsArgs a)
{
    __shared__ float tab[MAXFFT];
    __shared__ float xs[TC * PITCH];
    __shared__ float s_m0[32 * MT], s_r[32 * MT];
    const int n = a.n_fft, mask = n - 1, nb = n >> 1, groups = nb / BINS_PER_WG;
    const int u = blockIdx.x / groups, g = blockIdx.x - u * groups;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int K = a.K;
    if (u >= a.n_utts) return;
    const long long o0 = a.offs[u], o1 = a.offs[u + 1];
    if (o0 < 0 || o1 <= o0 || o1 > a.n_frames || o1 - o0 > n) return;       // (uniform) what the host checked, checked again: nothing is read
    const int T = (int)(o1 - o0);
    const float Tf = (float)T;
    const float* const cep = a.cep + o0;

    for (int i = tid; i < n; i += NTHREADS) tab[i] = a.table[i];
    for (int k = wave; k < 32 * MT; k += WAVES) {                           // (k is uniform in a wave)
        float m0 = 0.0f, r = 0.0f;
        if (k < K) {
            const float* row = cep + (long long)k * a.n_frames;
            // lane l takes t = l, l + 64, .. in order; sixteen loads are in flight per lane, the additions keep their order
            auto lane_chain = [&](auto term) {
                float s = 0.0f;
                for (int tb = lane; tb < T; tb += 64 * 16) {
                    float c[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j) c[j] = tb + 64 * j < T ? row[tb + 64 * j] : 0.0f;
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        if (tb + 64 * j < T) s = term(s, c[j]);
                }
                return wave_sum(s);
            };
            m0 = __fdiv_rn(lane_chain([](float s, float c) { return __fadd_rn(s, c); }), Tf);
            r = __fdiv_rn(lane_chain([m0](float s, float c) { return __fadd_rn(s, __fsub_rn(c, m0)); }), Tf);
            const float v = __fdiv_rn(lane_chain([m0, r](float s, float c) { const float x = __fsub_rn(__fsub_rn(c, m0), r); return fmaf(x, x, s); }), Tf);
            if (g == 0 && lane == 0) { a.mean[(long long)u * K + k] = __fadd_rn(m0, r); a.var[(long long)u * K + k] = v; }
        }
        if (lane == 0) { s_m0[k] = m0; s_r[k] = r; }
    }

    const int f = g * BINS_PER_WG + wave * 32 + l31 + 1;                    // 1 .. n_fft / 2
    const int step2f = (2 * f) & mask, quarter = n >> 2;
    const float* const xa = xs + half * PITCH + l31;
    f32x16 tre[MT], tim[MT];
    __builtin_memset(tre, 0, sizeof(tre));
    __builtin_memset(tim, 0, sizeof(tim));
    // Staging: thread tid owns frame tt = tid & 63 of rows (tid >> 6) + 4 j.  The loads of chunk c + 1 fly under the MFMAs of chunk c; they
    // read a clamped (row, frame) of the utterance itself, and what lies beyond K or T is replaced by zero when it is put into LDS.
    constexpr int NS = 32 * MT * TC / NTHREADS;
    const int s_tt = tid & (TC - 1), s_k0 = tid >> 6;
    float stage[NS];
    auto fetch = [&](int t0) {
        const int tc = t0 + min(s_tt, T - t0 - 1);
#pragma unroll
        for (int j = 0; j < NS; ++j) stage[j] = cep[(long long)min(s_k0 + WAVES * j, K - 1) * a.n_frames + tc];
    };
    auto put = [&](int t0) {
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int k = s_k0 + WAVES * j;
            const float v = __fsub_rn(__fsub_rn(stage[j], s_m0[k]), s_r[k]);
            xs[s_tt * PITCH + k] = (k < K && t0 + s_tt < T) ? v : 0.0f;
        }
    };
    fetch(0);
    for (int t0 = 0; t0 < T; t0 += TC) {
        __syncthreads();                                                     // the chunk before has been consumed (first time: table and row statistics are there)
        const int nt = min(TC, T - t0);
        put(t0);
        __syncthreads();
        if (t0 + TC < T) fetch(t0 + TC);
        f32x16 pre[MT], pim[MT];
        __builtin_memset(pre, 0, sizeof(pre));
        __builtin_memset(pim, 0, sizeof(pim));
        int ph = (f * (t0 + half)) & mask;                                   // f t < 2^23: exact
        const int nsteps = (nt + 1) >> 1;                                    // (an odd chunk's last frame pairs with a staged zero)
        float c = tab[ph], sn = tab[(ph + quarter) & mask], x[MT];          // operands of step s + 1 are read under the MFMAs of step s
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) x[mt] = xa[32 * mt];
        for (int s = 0; s < nsteps; ++s) {
            ph = (ph + step2f) & mask;
            const int sn_ = s + 1 < nsteps ? s + 1 : s;                      // (the last one is a repeat nobody uses)
            const float c2 = tab[ph], sn2 = tab[(ph + quarter) & mask];
            float x2[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) x2[mt] = xa[2 * sn_ * PITCH + 32 * mt];
            __builtin_amdgcn_sched_barrier(0);                               // (left alone, the reads sink to just before their use)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                pre[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[mt], c, pre[mt], 0, 0, 0);
                pim[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[mt], sn, pim[mt], 0, 0, 0);
            }
            c = c2; sn = sn2;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) x[mt] = x2[mt];
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) { tre[mt] += pre[mt]; tim[mt] += pim[mt]; }
    }

    const int nbins = nb;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * half;       // accumulator register r of this lane: row k, column f
            if (k < K) {
                const float re = tre[mt][r], im = tim[mt][r];
                a.power[((long long)u * K + k) * nbins + (f - 1)] = __fdiv_rn(fmaf(re, re, __fmul_rn(im, im)), Tf);
            }
        }
}

__global__ __launch_bounds__(NTHREADS) void ms_mean_log_kernel(const float* __restrict__ v, int n, long long R, float floor, float* __restrict__ out)
{
    const long long r = (long long)blockIdx.x * NTHREADS + threadIdx.x;
    if (r >= R) return;
    float s = 0.0f;
    for (int u = 0; u < n; ++u) {
        float x = v[(long long)u * R + r];
        if (x < floor) x = floor;                                            // (a NaN stays a NaN)
        s = __fadd_rn(s, __fmul_rn(10.0f, log10f(x)));
    }
    out[r] = __fdiv_rn(s, (float)n);
}

__global__ __launch_bounds__(NTHREADS) void ms_distance_kernel(const float* __restrict__ a, const float* __restrict__ b, int K, int nb, int F,
                                                               float* __restrict__ per_dim, float* __restrict__ total)
{
    __shared__ float S[MAXK];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = wave; k < K; k += WAVES) {
        float s = 0.0f;
        for (int f = lane; f < F; f += 64) { const float d = __fsub_rn(a[(long long)k * nb + f], b[(long long)k * nb + f]); s = fmaf(d, d, s); }
        s = wave_sum(s);
        if (lane == 0) { S[k] = s; per_dim[k] = sqrtf(__fdiv_rn(s, (float)F)); }
    }
    __syncthreads();
    if (wave == 0) {
        float s = 0.0f;
        for (int k = lane; k < K; k += 64) s = __fadd_rn(s, S[k]);
        s = wave_sum(s);
        if (lane == 0) total[0] = sqrtf(__fdiv_rn(s, (float)K * (float)F));
    }
}

bool fft_ok(int n_fft) { return n_fft == 1024 || n_fft == 2048 || n_fft == 4096; }

}  // namespace

int mcvc_ms_table_fill(int n_fft, float* host)
{
    if (!fft_ok(n_fft) || !host) return MCVC_ERR_INVALID;
    for (int j = 0; j < n_fft; ++j) host[j] = (float)std::cos(2.0 * kPi * j / n_fft);
    return MCVC_OK;
}

int mcvc_ms_power_launch(const float* cep, long long n_frames, int K, const int* offs_dev, int n_utts, const int* offs_host, int n_fft,
                         const float* table, float* power, float* mean, float* var, hipStream_t s)
{
    if (!cep || !offs_dev || !offs_host || !table || !power || !mean || !var) return MCVC_ERR_INVALID;
    if (((uintptr_t)cep & 3) || ((uintptr_t)offs_dev & 3) || ((uintptr_t)offs_host & 3) || ((uintptr_t)table & 15) || ((uintptr_t)power & 3) ||
        ((uintptr_t)mean & 3) || ((uintptr_t)var & 3)) return MCVC_ERR_INVALID;
    if (K < 1 || K > MAXK || !fft_ok(n_fft) || n_utts < 1 || n_frames < 1 || n_frames > 0x7fffffffLL) return MCVC_ERR_INVALID;
    if (offs_host[0] != 0 || offs_host[n_utts] != n_frames) return MCVC_ERR_INVALID;
    for (int u = 0; u < n_utts; ++u) {
        const long long T = (long long)offs_host[u + 1] - offs_host[u];
        if (T < 1 || T > n_fft) return MCVC_ERR_INVALID;                     // (also: offsets that do not rise)
    }
    const int groups = (n_fft / 2) / BINS_PER_WG;
    if ((long long)n_utts * groups > 0x7fffffffLL) return MCVC_ERR_INVALID;
    MsArgs a{};
    a.cep = cep; a.offs = offs_dev; a.table = table; a.power = power; a.mean = mean; a.var = var;
    a.n_frames = n_frames; a.K = K; a.n_utts = n_utts; a.n_fft = n_fft;
    TraceScope ts(K_SGEMM, s, 4.0 * K * (double)n_frames * (n_fft / 2), 4.0 * K * ((double)n_frames * groups + (double)n_utts * (n_fft / 2)));
    const dim3 grid((unsigned)(n_utts * groups)), block(NTHREADS);
    switch ((K + 31) / 32) {
        case 1: hipLaunchKernelGGL(ms_power_kernel<1>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(ms_power_kernel<2>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(ms_power_kernel<3>, grid, block, 0, s, a); break;
    }
    return (int)hipGetLastError();
}

int mcvc_ms_mean_log_launch(const float* values, int n, long long R, float floor, float* out, hipStream_t s)
{
    if (!values || !out || ((uintptr_t)values & 3) || ((uintptr_t)out & 3)) return MCVC_ERR_INVALID;
    if (n < 1 || R < 1 || cdiv_ll(R, NTHREADS) > 0x7fffffffLL || !(floor > 0.0f) || !std::isfinite(floor)) return MCVC_ERR_INVALID;
    TraceScope ts(K_ELEMENTWISE, s, 3.0 * n * (double)R, 4.0 * (n + 1) * (double)R);
    hipLaunchKernelGGL(ms_mean_log_kernel, dim3((unsigned)cdiv_ll(R, NTHREADS)), dim3(NTHREADS), 0, s, values, n, R, floor, out);
    return (int)hipGetLastError();
}

int mcvc_ms_distance_launch(const float* a, const float* b, int K, int n_bins, int n_used, float* per_dim, float* total, hipStream_t s)
{
    if (!a || !b || !per_dim || !total || ((uintptr_t)a & 3) || ((uintptr_t)b & 3) || ((uintptr_t)per_dim & 3) || ((uintptr_t)total & 3)) return MCVC_ERR_INVALID;
    if (K < 1 || K > MAXK || n_bins < 1 || n_bins > MAXFFT / 2 || n_used < 1 || n_used > n_bins) return MCVC_ERR_INVALID;
    TraceScope ts(K_ELEMENTWISE, s, 3.0 * K * (double)n_used, 8.0 * K * (double)n_used);
    hipLaunchKernelGGL(ms_distance_kernel, dim3(1), dim3(NTHREADS), 0, s, a, b, K, n_bins, n_used, per_dim, total);
    return (int)hipGetLastError();
}
