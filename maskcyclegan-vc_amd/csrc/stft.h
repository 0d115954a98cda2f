// The STFT tile engine: the one definition of how the project's short-time Fourier transform (reflect-pad 384, frames of 1024 at hop 256,
// periodic Hann, bins 0..512) is tiled on v_mfma_f32_32x32x2_f32.  The front-end (audio_kernels.hip) and the Griffin-Lim decoder
// (griffinlim_kernels.hip) are loaders and epilogues around it, so the decoder's forward transform IS the front-end's.
//
// A workgroup of eight waves owns 64 consecutive frames of one utterance.  Their samples are staged in LDS once, with one float of skew
// per 256 (frame n starts at 257 n: conflict-free B reads), and multiplied with a [1024 rows][1024 k] basis that streams from L2 straight
// to registers, pre-arranged on the host in the order the lanes consume it:
//   float index ((mt * 128 + kg) * 64 + lane) * 4 + j  =  W[k = 8 kg + 2 j + (lane >> 5)][row 32 mt + (lane & 31)]
// -- one coalesced 16-byte load per lane, row tile and eight k.
#pragma once
#include "audio.h"
#include "mcvc_common.h"

#include <cmath>
#include <vector>

namespace stft {

constexpr int HOP = MCVC_AUDIO_HOP, NFFT = MCVC_AUDIO_NFFT, PAD = MCVC_AUDIO_PAD, NBIN = NFFT / 2 + 1, NMEL = MCVC_AUDIO_NMEL;
constexpr int TF = MCVC_AUDIO_TILE_FRAMES;                 // frames per workgroup
constexpr int NTHREADS = 512;                              // eight waves split the basis' row tiles
constexpr int SPAN = (TF - 1) * HOP + NFFT;                // samples the frames of a tile cover
constexpr int PITCH = HOP + 1;                             // floats from one staged frame (or column) to the next
constexpr int SPAN_LDS = SPAN + SPAN / 256 + 1;            // stored with one float of skew per 256: frame n starts at 257 n
constexpr int KG = NFFT / 8;                               // k groups of 8 (one 16-byte basis load per lane and row tile)
constexpr long long DFT_FLOATS = (long long)NFFT * NFFT;   // 1024 rows x 1024 k
static_assert(HOP == 256 && NFFT % HOP == 0 && TF == 64, "the skew of one float per 256 puts frame n at 257 n; a tile is two MFMA column tiles");
static_assert(SPAN - 1 + ((SPAN - 1) >> 8) < SPAN_LDS && PITCH * (TF - 1) + NFFT - 1 + ((NFFT - 1) >> 8) < SPAN_LDS, "the stage holds every frame");
static_assert(NFFT % 32 == 0 && KG % 2 == 0, "whole row tiles, k groups in pairs");

template <int MT>
__device__ __forceinline__ void stft_zero(f32x16 (&acc)[MT][2]) { __builtin_memset(acc, 0, sizeof(acc)); }

// The samples of frames t0 .. t0 + nv - 1 of a signal of L samples, reflected at the signal's own two ends (F.pad 'reflect': the edge
// sample is not repeated), skewed into smem; the rest of the stage is zero.  sample(i) is the signal at 0 <= i < L.
template <class Sample>
__device__ __forceinline__ void stft_stage_tile(float* smem, int t0, int nv, int L, Sample sample)
{
    const int p0 = t0 * HOP - PAD;                          // index in the signal of the tile's first padded sample
    const int s_end = (nv - 1) * HOP + NFFT;                // samples the valid frames cover
    for (int s = threadIdx.x; s < SPAN; s += NTHREADS) {
        float v = 0.f;
        if (s < s_end) {
            int i = p0 + s;
            if (i < 0) i = -i;
            if (i >= L) i = 2 * (L - 1) - i;
            if (i >= 0 && i < L) v = sample(i);             // (always true for a valid frame: L >= 385 > 384)
        }
        smem[s + (s >> 8)] = v;
    }
    __syncthreads();
}

// What a lane reads as the B operand: column l31 = lane & 31 of a stage of PITCH floats per column, k parity half = lane >> 5.
__device__ __forceinline__ const float* stft_b_lane(const float* smem, int l31, int half) { return smem + PITCH * l31 + half; }

// tot[mt][nt] += row tiles mt of a lane-ordered basis (ap: the wave's first) x the 64 columns staged at PITCH floats each, k groups kg0 ..
// kg0 + nkg - 1 (b_lane0: stft_b_lane at the FIRST of those groups; SKEW: the stage keeps one float of skew per 256 k).  Two register
// stages of the basis are filled one k group ahead: a wave's loads of group kg + 1 fly under its MFMAs of group kg.
// FLUSH_KG == 0: one chain into tot, the front-end's.
// FLUSH_KG > 0: an MFMA chain is a k-ordered fmaf chain, and a straight sum of 1024 terms is ~3.6x further from float64 than an FFT
// (measured: 5.7e-7 against 1.5e-7 rel-L2 for one inverse transform).  So every FLUSH_KG k groups (4: 32 terms) are summed from zero in
// accumulators of their own and then added to the running total -- chains of 32 + 32 instead of 1024, the two levels of the decoder's GEMM.
template <int MT, int FLUSH_KG, bool SKEW>
__device__ __forceinline__ void stft_product(f32x16 (&tot)[MT][2], const f32x4* __restrict__ ap, const float* b_lane0, int kg0, int nkg)
{
    static_assert(FLUSH_KG % 2 == 0, "k groups go in pairs");
    const float* const b_lane1 = b_lane0 + PITCH * 32;
    f32x4 st0[MT], st1[MT];
    f32x16 part[MT][2];
    f32x16 (&acc)[MT][2] = FLUSH_KG ? part : tot;
    auto fetch = [&](f32x4 (&st)[MT], int kg) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) st[mt] = ap[((long long)mt * KG + kg) * 64];
    };
    auto multiply = [&](const f32x4 (&st)[MT], int kl) {
        const int kb = 8 * kl + (SKEW ? (kl >> 5) : 0);     // k = 8 kl + 2 j + half sits at 257 n + k + (k >> 8)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float b0 = b_lane0[kb + 2 * j], b1 = b_lane1[kb + 2 * j];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                acc[mt][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(st[mt][j], b0, acc[mt][0], 0, 0, 0);
                acc[mt][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(st[mt][j], b1, acc[mt][1], 0, 0, 0);
            }
        }
    };
    auto pair = [&](int kl) {
        fetch(st1, kg0 + kl + 1);
        __builtin_amdgcn_sched_barrier(0);                  // (left alone, the scheduler sinks the loads to half a group before their use)
        multiply(st0, kl);
        fetch(st0, kl + 2 < nkg ? kg0 + kl + 2 : kg0 + kl); // (the last one is a repeat nobody uses)
        __builtin_amdgcn_sched_barrier(0);
        multiply(st1, kl + 1);
    };
    fetch(st0, kg0);
    if constexpr (FLUSH_KG == 0) {
#pragma unroll 1
        for (int kl = 0; kl < nkg; kl += 2) pair(kl);
    } else {
#pragma unroll 1
        for (int kf = 0; kf < nkg; kf += FLUSH_KG) {
            stft_zero(part);
#pragma unroll
            for (int kl = kf; kl < kf + FLUSH_KG; kl += 2) pair(kl);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) tot[mt][nt] += part[mt][nt];
        }
    }
}

// Where a product lands.  With p = stft_pair(rt, q, lane >> 5), rt the row tile that mt stands for, registers 4 q .. 4 q + 3 (q = 0..3) of
// acc[mt][nt] hold rows 2 p .. 2 p + 3 of the basis in column stft_col(lane & 31, nt) of the stage: a lane has four runs of four consecutive
// rows of one column.  Where rows (2 b, 2 b + 1) are (re, im) of bin b, those are bins p and p + 1.
__device__ __forceinline__ int stft_pair(int rt, int q, int half) { return 16 * rt + 4 * q + 2 * half; }
__device__ __forceinline__ int stft_col(int l31, int nt) { return l31 + 32 * nt; }

// ---- host: the tables a basis is made of, in float64, and the lane order ----
constexpr double kPi = 3.14159265358979323846;

struct Tables {
    std::vector<double> hann, cs, sn;                       // periodic Hann (torch.hann_window), cos and sin of 2 pi k / 1024
    Tables() : hann(NFFT), cs(NFFT), sn(NFFT)
    {
        for (int k = 0; k < NFFT; ++k) {
            hann[k] = 0.5 - 0.5 * std::cos(2.0 * kPi * k / NFFT);
            cs[k] = std::cos(2.0 * kPi * k / NFFT);
            sn[k] = std::sin(2.0 * kPi * k / NFFT);
        }
    }
};

// index into cs / sn of the angle 2 pi a b / 1024: exact argument reduction
inline int stft_phase(int a, int b) { return (int)(((long long)a * b) % NFFT); }

// out[DFT_FLOATS] in the lanes' order (file header) from element(k, row) in float64
template <class Element>
inline void stft_fill_lane_order(float* out, Element element)
{
    for (int mt = 0; mt < NFFT / 32; ++mt)
        for (int kg = 0; kg < KG; ++kg)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int k = 8 * kg + 2 * j + (lane >> 5), row = 32 * mt + (lane & 31);
                    out[(((long long)mt * KG + kg) * 64 + lane) * 4 + j] = (float)element(k, row);
                }
}

}  // namespace stft
