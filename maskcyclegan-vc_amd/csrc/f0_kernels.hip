// Pitch tracking: YIN (de Cheveigne & Kawahara 2002) on the mel front-end's frame grid, and F0 statistics along DTW paths (definitions:
// mask_cyclegan_vc/pitch.py; tests/f0_checker.py restates them in float64).
//
//   f0_track_kernel   one workgroup per SUB-TILE: eight consecutive frames of one utterance (a tile of mcvc_audio_plan is cut into eight).
//                     Frame t is centred on sample c_t = 256 t + 128 and integrates buf[j] = x[s_t + j], s_t = c_t - (W + tau_max) / 2, with zeros
//                     outside the utterance, so a term (x[g] - x[g + tau])^2 depends on the position g alone and neighbouring frames share 3/4
//                     of their terms.  The sub-tile's samples (x[s_first ..], 11 hops + the lags) are staged in LDS once; the span is cut into
//                     hop-sized BLOCKS b = 0 .. frames + 2 and
//                         E_b(tau) = sum_{256 b <= p < 256 b + 256} (xs[p] - xs[p + tau])^2,     d_f(tau) = ((E_f + E_f+1) + E_f+2) + E_f+3:
//                     11 blocks instead of 8 x 4 -- the difference function costs 2.9 x fewer operations than frame by frame, it is still
//                     computed from differences, and a frame's sum has one order whatever shares the sub-tile with it.
//                     A lane owns FOUR consecutive lags 4 l .. 4 l + 3 and walks a block four positions at a time: two 16-byte LDS reads (the
//                     positions, the same address in every lane; the next four shifted samples, consecutive across lanes: no bank conflict)
//                     feed 16 subtract / fused multiply-adds.  ceil((tau_max + 1) / 4) lanes are busy: 64, 128 or 192 threads per workgroup,
//                     chosen at the launch.  d stays in LDS (it takes the samples' place): a wave per frame sums lags in 64 contiguous chunks
//                     (chunk sums, one wave scan, then the running sum inside the chunk), overwrites d with d' = d tau / running sum and makes
//                     the pick on those stored float32 values: ballot for the first lag under the threshold, the descent, the parabola.
//   f0_stats_kernel   one wavefront per pair over the rows of its DTW path: lane l takes rows l, l + 64, ... in order, then a butterfly.
// No atomics, no scratch, no device allocation; every trip count is a function of the lengths and the lag range alone.
#include <cmath>
#include <cstdint>
#include <limits>

#include "audio.h"
#include "f0.h"
#include "mcvc_common.h"
#include "trace.h"

namespace {

constexpr int W = MCVC_F0_WINDOW, HOP = MCVC_AUDIO_HOP, MAXLAG = MCVC_F0_MAX_LAG, FS = MCVC_F0_SUB_FRAMES, TF = MCVC_AUDIO_TILE_FRAMES;
constexpr int NBLK = FS + W / HOP - 1;                         // 11 blocks of one hop cover eight windows
constexpr int MAXTHREADS = 192;                                // 4 lags per lane: 768 >= MAXLAG + 1
constexpr int XS = NBLK * HOP + 4 * MAXTHREADS + 8;            // staged samples: the last lane's window read stays inside
constexpr int DPITCH = MAXLAG + 4;                             // floats of d per frame (lags 0 .. 643: whole groups of four)
constexpr int SMEM = XS > FS * DPITCH ? XS : FS * DPITCH;      // 20.1 KB: d takes the samples' place
constexpr float RATE = (float)MCVC_AUDIO_RATE;
static_assert(4 * MAXTHREADS >= MAXLAG + 1 && (DPITCH % 4) == 0 && W % HOP == 0 && TF % FS == 0, "f0 tiling");

struct F0Args {
    const float* wave;
    const int* tiles;          // mcvc_audio_plan's work list: first sample of the utterance, its length, output column of the tile's first frame, first frame
    float* f0; float* ap;      // [total_frames]
    float* cmnd;               // [tau_max + 1][total_frames] or null
    long long n_samples, total_frames;
    float thr;
    int tau_min, tau_max;
};

__global__ __launch_bounds__(MAXTHREADS) void f0_track_kernel(const F0Args a)
{
    __shared__ __attribute__((aligned(16))) float smem[SMEM];
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nthr >> 6;
    const BankTile tile(a.tiles, a.n_samples, a.total_frames);
    const long long s0 = tile.s0, col0 = tile.col0;
    const int L = tile.L, t0 = tile.t0;
    const int fb = FS * blockIdx.y;                             // the sub-tile's first frame inside the tile
    if (tile.nv - fb < 1) return;                               // (uniform: the whole workgroup leaves before its first barrier)
    const int nvf = tile.nv - fb < FS ? tile.nv - fb : FS;
    const int tau_min = a.tau_min, tau_max = a.tau_max;

    // ---- the sub-tile's samples; outside [0, L) of this utterance they are zero, never the neighbour's ----
    const float* const src = a.wave + s0;
    const long long g0 = (long long)(t0 + fb) * HOP + HOP / 2 - (W + tau_max) / 2;
    for (int i = tid; i < XS; i += nthr) {
        const long long g = g0 + i;
        smem[i] = (g >= 0 && g < L) ? src[g] : 0.f;
    }
    __syncthreads();

    // ---- difference function: d[f][k] = d_f(4 tid + k) ----
    const int tau0 = 4 * tid;
    const bool busy = tau0 <= tau_max;
    const int nblk = nvf + W / HOP - 1;
    f32x4 d[FS];
#pragma unroll
    for (int f = 0; f < FS; ++f) d[f] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (busy) {
#pragma unroll
        for (int b = 0; b < NBLK; ++b) {
            if (b < nblk) {                                     // (uniform)
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                const float* const xa = smem + HOP * b;
                const float* const xv = xa + tau0;
                f32x4 lo = *reinterpret_cast<const f32x4*>(xv);
#pragma unroll 2
                for (int p = 0; p < HOP; p += 4) {
                    const f32x4 av = *reinterpret_cast<const f32x4*>(xa + p);
                    const f32x4 hi = *reinterpret_cast<const f32x4*>(xv + p + 4);
                    const float w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                    for (int i = 0; i < 4; ++i)                 // positions in rising order: one summation order per lag
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float diff = av[i] - w[i + k];
                            acc[k] = fmaf(diff, diff, acc[k]);
                        }
                    lo = hi;
                }
#pragma unroll
                for (int f = 0; f < FS; ++f)
                    if (f <= b && b < f + W / HOP) d[f] += acc; // (decided at compile time: d is never indexed at run time)
            }
        }
    }
    __syncthreads();                                            // every wave is done with the samples: d takes their place
    if (busy) {
#pragma unroll
        for (int f = 0; f < FS; ++f) *reinterpret_cast<f32x4*>(smem + f * DPITCH + tau0) = d[f];
    }
    __syncthreads();

    // ---- cumulative-mean normalisation, in place: a wave per frame, lane l owns lags 1 + l C .. (l + 1) C ----
    const int C = (tau_max + 63) >> 6;
    for (int f = wave; f < nvf; f += nwaves) {
        float* const dl = smem + f * DPITCH;
        const int t_lo = 1 + lane * C, t_hi = min(tau_max, t_lo + C - 1);
        float inc = 0.f;
        for (int t = t_lo; t <= t_hi; ++t) inc += dl[t];
        for (int o = 1; o < 64; o <<= 1) {
            const float v = __shfl_up(inc, o);
            if (lane >= o) inc += v;
        }
        float run = __shfl_up(inc, 1);
        if (lane == 0) run = 0.f;
        for (int t = t_lo; t <= t_hi; ++t) {
            const float dv = dl[t];
            run += dv;
            dl[t] = run > 0.f ? dv * (float)t / run : 1.f;      // (d >= 0: the sum is 0 only where every term is)
        }
        if (lane == 0) dl[0] = 1.f;
    }
    __syncthreads();

    if (a.cmnd) {                                               // the values the pick is made on
        const int n = (tau_max + 1) * nvf;
        for (int idx = tid; idx < n; idx += nthr) {
            const int t = idx / nvf, f = idx - t * nvf;
            a.cmnd[(long long)t * a.total_frames + col0 + fb + f] = smem[f * DPITCH + t];
        }
    }

    // ---- pick ----
    const float INF = std::numeric_limits<float>::infinity();
    for (int f = wave; f < nvf; f += nwaves) {
        const float* const dl = smem + f * DPITCH;
        int tau = -1;
        float mn = INF;
        for (int base = tau_min; base <= tau_max; base += 64) {
            const int t = base + lane;
            const float v = t <= tau_max ? dl[t] : INF;
            mn = fminf(mn, v);
            const unsigned long long under = __ballot(v < a.thr);
            if (under) { tau = base + __ffsll(under) - 1; break; }
        }
        float f0v = 0.f, apv;
        if (tau >= 0) {                                         // (uniform: tau comes from the ballot)
            while (tau + 1 <= tau_max && dl[tau + 1] < dl[tau]) ++tau;
            const float bq = dl[tau];
            float off = 0.f;
            if (tau < tau_max) {
                const float aq = dl[tau - 1], cq = dl[tau + 1];
                const float den = (aq - bq) + (cq - bq);
                if (den > 0.f) off = fminf(fmaxf(0.5f * (aq - cq) / den, -0.5f), 0.5f);
            }
            f0v = RATE / ((float)tau + off);
            apv = bq;
        } else {
            for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o));
            apv = mn;
        }
        if (lane == 0) {
            a.f0[col0 + fb + f] = f0v;
            a.ap[col0 + fb + f] = apv;
        }
    }
}

struct F0StatArgs {
    const float* fx; const float* fy;
    const int* path;           // [rows][2] as mcvc_dtw_run wrote it
    const long long* pairs;    // [n_pairs][4]
    int* counts; float* sums;
    long long nx, ny;
};

__global__ __launch_bounds__(64) void f0_stats_kernel(const F0StatArgs a)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    const long long* const r = a.pairs + (long long)MCVC_F0_PAIR_COLS * p;
    const long long xo = r[0], yo = r[1], po = r[2], n = r[3];
    int c_both = 0, c_x = 0, c_y = 0, c_none = 0;
    float s1 = 0.f, s2 = 0.f;
    // a row of the table that does not describe these banks counts nothing; a path row that points outside them is skipped
    const bool ok = xo >= 0 && xo < a.nx && yo >= 0 && yo < a.ny && po >= 0 && n >= 0 && n <= 0x7fffffffLL;
    if (ok) {
        const int2* const rows = reinterpret_cast<const int2*>(a.path) + po;
        for (long long k = lane; k < n; k += 64) {
            const int2 ij = rows[k];
            if (ij.x < 0 || ij.y < 0 || xo + ij.x >= a.nx || yo + ij.y >= a.ny) continue;
            const float u = a.fx[xo + ij.x], v = a.fy[yo + ij.y];
            const bool vu = u > 0.f, vv = v > 0.f;
            if (vu && vv) {
                const float c = __fmul_rn(1200.f, log2f(u / v));          // cents
                ++c_both; s1 += c; s2 = fmaf(c, c, s2);
            } else if (vu) ++c_x;
            else if (vv) ++c_y;
            else ++c_none;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {                          // both partners add the same two numbers: every lane ends with one result
        c_both += __shfl_xor(c_both, o); c_x += __shfl_xor(c_x, o); c_y += __shfl_xor(c_y, o); c_none += __shfl_xor(c_none, o);
        s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o);
    }
    if (lane == 0) {
        int* const c = a.counts + 4LL * p;
        c[0] = c_both; c[1] = c_x; c[2] = c_y; c[3] = c_none;
        a.sums[2LL * p] = s1; a.sums[2LL * p + 1] = s2;
    }
}

}  // namespace

int mcvc_f0_track_launch(const float* wave, long long n_samples, const int* tiles, int n_tiles, int tau_min, int tau_max, float threshold,
                         float* f0, float* aperiodicity, float* cmnd, long long total_frames, hipStream_t s)
{
    if (!wave || !tiles || !f0 || !aperiodicity || n_samples < MCVC_AUDIO_PAD + 1 || n_tiles < 1 || total_frames < 1 || total_frames > 0x7fffffffLL) return MCVC_ERR_INVALID;
    if (((uintptr_t)wave & 3) || ((uintptr_t)f0 & 3) || ((uintptr_t)aperiodicity & 3) || ((uintptr_t)cmnd & 3) || ((uintptr_t)tiles & 15)) return MCVC_ERR_INVALID;
    if (!(tau_min >= 2 && tau_min < tau_max && tau_max <= MAXLAG)) return MCVC_ERR_INVALID;
    if (!(threshold > 0.f && threshold <= 1.f)) return MCVC_ERR_INVALID;              // (a NaN fails both comparisons)
    const F0Args a{wave, tiles, f0, aperiodicity, cmnd, n_samples, total_frames, threshold, tau_min, tau_max};
    const int threads = 64 * cdiv_i(cdiv_i(tau_max + 1, 4), 64);
    const double terms = (double)total_frames * NBLK / FS * HOP * (tau_max + 1);
    TraceScope ts(K_ELEMENTWISE, s, 3.0 * terms, 4.0 * n_samples + 8.0 * total_frames + (cmnd ? 4.0 * (tau_max + 1) * (double)total_frames : 0.0));
    hipLaunchKernelGGL(f0_track_kernel, dim3((unsigned)n_tiles, TF / FS), dim3(threads), 0, s, a);
    return (int)hipGetLastError();
}

int mcvc_f0_stats_launch(const float* fx, long long x_frames, const float* fy, long long y_frames, const int* path, const long long* pairs,
                         int n_pairs, int* counts, float* sums, hipStream_t s)
{
    if (!fx || !fy || !path || !pairs || !counts || !sums || x_frames < 1 || y_frames < 1 || n_pairs < 1) return MCVC_ERR_INVALID;
    if (((uintptr_t)fx & 3) || ((uintptr_t)fy & 3) || ((uintptr_t)counts & 3) || ((uintptr_t)sums & 3) || ((uintptr_t)path & 7) || ((uintptr_t)pairs & 15))
        return MCVC_ERR_INVALID;
    const F0StatArgs a{fx, fy, path, pairs, counts, sums, x_frames, y_frames};
    TraceScope ts(K_ELEMENTWISE, s, 0.0, 40.0 * n_pairs);
    hipLaunchKernelGGL(f0_stats_kernel, dim3((unsigned)n_pairs), dim3(64), 0, s, a);
    return (int)hipGetLastError();
}
