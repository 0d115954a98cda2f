// Waveform -> log-mel front-end (the MelGAN vocoder's Audio2Mel transform, which the reference fetches through torch.hub in
// data_preprocessing/preprocess_vcc2018.py and mask_cyclegan_vc/utils.py): one fused launch from a bank of waveforms to a bank of
// log-mel-spectrograms.
//
//   reflect-pad 384 | frames of 1024 at hop 256 | periodic Hann | DFT bins 0..512 | magnitude | 80 x 513 Slaney mel basis | log10(max(., 1e-5))
//
// The transform is a matrix product.  The frame matrix of an utterance is its padded audio read with a row stride of 256 samples; a
// workgroup stages the samples of 64 consecutive frames of ONE utterance in LDS once (63 * 256 + 1024 floats; the reflection at the
// utterance's own two ends is index arithmetic at that point, so a neighbour in the bank is never read) and multiplies them with the
// windowed cos / sin basis on v_mfma_f32_32x32x2_f32:  M = basis column (1024), N = frame (64), K = sample in frame (1024).  The tile's
// constants, the reflected loader, the product and the accumulator mapping are the STFT tile engine's (stft.h), which the Griffin-Lim
// decoder shares; this file adds the basis' element formula and the magnitude / mel / log epilogue.
//
// Basis layout (mcvc_audio_basis_init).  Column 2b is hann * cos and column 2b + 1 hann * sin of bin b = 0..511, so accumulator rows
// (2b, 2b + 1) of a lane are the real and imaginary part of one (bin, frame): the magnitude needs no cross-lane traffic.  The sine column
// of bin 0 is identically zero; it carries the cosine column of bin 512 (Nyquist, hann * (-1)^k, whose sine is zero as well) instead, so
// 513 bins fit 1024 columns = 32 MFMA row tiles, four per wave.  The eight waves split M, so every basis element is used by exactly one
// wave of a workgroup: it goes from L2 straight to registers (no LDS), in the lane order of stft.h.
//
// The spectrum never leaves the chip: magnitudes go to LDS ([513][64], over the dead sample stage), the 513 -> 80 mel product runs from
// there (each bin feeds at most two filters: per filter a contiguous bin range and its weights, summed in ascending bin order by one
// thread per (filter, frame) -- no atomics, so a frame's value does not depend on what else is in the launch), then log10 / clamp and a
// store of 64 consecutive floats per mel row.
#include "mcvc_common.h"
#include "stft.h"
#include "trace.h"

#include <cmath>
#include <mutex>
#include <vector>

namespace {

using namespace stft;

constexpr int MAG_FLOATS = NBIN * TF;
constexpr int LDS_FLOATS = MAG_FLOATS > SPAN_LDS ? MAG_FLOATS : SPAN_LDS;
constexpr int MT_PER_WAVE = 4;                             // eight waves split the 32 row tiles: 128 accumulator registers each, two waves per SIMD
constexpr int TAB_HEAD = 256;                              // int32 lo[80] | count[80] | weight offset[80] | pad

struct AudioArgs {
    const float* wave;
    const int* tiles;          // [n_tiles][4] = first sample of the utterance, its length, output column of the tile's first frame, first frame in the utterance
    const float* basis;
    float* out;                // [80][total_frames]
    long long n_samples, total_frames;
};

__global__ void __launch_bounds__(NTHREADS) audio_log_mel_kernel(const AudioArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const BankTile tile(a.tiles, a.n_samples, a.total_frames);
    const long long col0 = tile.col0;
    const int nv = tile.nv;
    if (nv < 1) return;

    // ---- the tile's samples, reflected at the utterance's own ends ----
    const float* const src = a.wave + tile.s0;
    stft_stage_tile(smem, tile.t0, nv, tile.L, [&](int i) { return src[i]; });

    // ---- spectrum: acc[mt][nt] = rows 32 (4 wave + mt) .. + 31 of the basis x frames 32 nt .. + 31 ----
    f32x16 acc[MT_PER_WAVE][2];
    stft_zero(acc);
    const f32x4* const ap = reinterpret_cast<const f32x4*>(a.basis) + (long long)wave * MT_PER_WAVE * KG * 64 + lane;
    stft_product<MT_PER_WAVE, 0, true>(acc, ap, stft_b_lane(smem, l31, half), 0, KG);
    __syncthreads();                                        // every wave is done with the samples: the magnitudes take their place

    // ---- magnitude: rows (2 bin, 2 bin + 1) = (re, im) of one bin ----
#pragma unroll
    for (int mt = 0; mt < MT_PER_WAVE; ++mt) {
        __builtin_amdgcn_sched_barrier(0);                  // (one row tile at a time)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    const float re = acc[mt][nt][4 * q + 2 * pr], im = acc[mt][nt][4 * q + 2 * pr + 1];
                    const int bin = stft_pair(wave * MT_PER_WAVE + mt, q, half) + pr;
                    const int n = stft_col(l31, nt);
                    if (bin == 0) {                         // (real DC, real Nyquist) share the pair
                        smem[n] = fabsf(re);
                        smem[(NBIN - 1) * TF + n] = fabsf(im);
                    } else
                        smem[bin * TF + n] = sqrtf(re * re + im * im);
                }
    }
    __syncthreads();

    // ---- mel product, log10, clamp, store ----
    const int* const head = reinterpret_cast<const int*>(a.basis + DFT_FLOATS);
    const float* const wts = a.basis + DFT_FLOATS + TAB_HEAD;
    const int n = tid & 63;
    for (int i = tid >> 6; i < NMEL; i += NTHREADS / 64) {
        const int lo = head[i], cnt = head[NMEL + i];
        const float* w = wts + head[2 * NMEL + i];
        float s = 0.f;
        for (int c = 0; c < cnt; ++c) s += w[c] * smem[(lo + c) * TF + n];
        if (n < nv) a.out[(long long)i * a.total_frames + col0 + n] = s > 1e-5f ? log10f(s) : -5.0f;
    }
}

// ---- host: the Slaney mel filterbank, in float64 ----
double hz_to_mel(double f)
{
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}

double mel_to_hz(double m)
{
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

struct MelTable {
    int lo[NMEL], cnt[NMEL], off[NMEL];
    std::vector<float> w;
};

const MelTable& mel_table()
{
    static MelTable t;
    static std::once_flag once;
    std::call_once(once, [] {
        const double fmax = MCVC_AUDIO_RATE / 2.0;
        double edge[NMEL + 2];
        const double m_hi = hz_to_mel(fmax);
        for (int i = 0; i < NMEL + 2; ++i) edge[i] = mel_to_hz(m_hi * i / (NMEL + 1));
        for (int i = 0; i < NMEL; ++i) {
            t.lo[i] = 0; t.cnt[i] = 0; t.off[i] = (int)t.w.size();
            int first = -1, last = -1;
            std::vector<float> row(NBIN);
            for (int b = 0; b < NBIN; ++b) {
                const double f = fmax * b / (NBIN - 1);
                const double up = (f - edge[i]) / (edge[i + 1] - edge[i]), down = (edge[i + 2] - f) / (edge[i + 2] - edge[i + 1]);
                double v = up < down ? up : down;
                v = (v > 0 ? v : 0) * 2.0 / (edge[i + 2] - edge[i]);
                row[b] = (float)v;
                if (row[b] != 0.f) { if (first < 0) first = b; last = b; }
            }
            if (first >= 0) {
                t.lo[i] = first; t.cnt[i] = last - first + 1;
                t.w.insert(t.w.end(), row.begin() + first, row.begin() + last + 1);
            }
        }
    });
    return t;
}

}  // namespace

int mcvc_audio_frames_of(int n_samples) { return n_samples < PAD + 1 ? 0 : (n_samples - HOP) / HOP + 1; }

long long mcvc_audio_basis_floats_of() { return DFT_FLOATS + TAB_HEAD + (long long)mel_table().w.size(); }

void mcvc_audio_basis_fill(float* out)
{
    const Tables w;
    stft_fill_lane_order(out, [&](int k, int m) {           // row m of the basis, sample k
        const int bin = m == 1 ? NFFT / 2 : m >> 1;         // row 1: the Nyquist cosine
        const int ph = stft_phase(k, bin);
        return w.hann[k] * ((m == 1 || !(m & 1)) ? w.cs[ph] : w.sn[ph]);
    });
    const MelTable& t = mel_table();
    int* head = reinterpret_cast<int*>(out + DFT_FLOATS);
    for (int i = 0; i < TAB_HEAD; ++i) head[i] = 0;
    for (int i = 0; i < NMEL; ++i) { head[i] = t.lo[i]; head[NMEL + i] = t.cnt[i]; head[2 * NMEL + i] = t.off[i]; }
    for (size_t i = 0; i < t.w.size(); ++i) out[DFT_FLOATS + TAB_HEAD + i] = t.w[i];
}

int mcvc_audio_plan_host(const int* sample_offs, int n_utts, int* frame_offs, int* tiles, int max_tiles, int* n_tiles_out)
{
    if (!sample_offs || n_utts < 1 || !frame_offs || !n_tiles_out || sample_offs[0] < 0) return MCVC_ERR_INVALID;
    long long frames = 0, nt = 0;
    for (int u = 0; u < n_utts; ++u) {
        const long long L = (long long)sample_offs[u + 1] - sample_offs[u];
        if (L < PAD + 1) return MCVC_ERR_INVALID;           // reflect padding needs more samples than it adds (torch raises too)
        const long long T = (L - HOP) / HOP + 1;
        frames += T; nt += (T + TF - 1) / TF;
    }
    if (frames > 0x7fffffffLL) return MCVC_ERR_INVALID;
    *n_tiles_out = (int)nt;
    if (tiles && nt > max_tiles) return MCVC_ERR_WORKSPACE;
    int f = 0, k = 0;
    for (int u = 0; u < n_utts; ++u) {
        const int L = sample_offs[u + 1] - sample_offs[u], T = mcvc_audio_frames_of(L);
        frame_offs[u] = f;
        for (int t0 = 0; tiles && t0 < T; t0 += TF, ++k) {
            tiles[4 * k] = sample_offs[u]; tiles[4 * k + 1] = L; tiles[4 * k + 2] = f + t0; tiles[4 * k + 3] = t0;
        }
        f += T;
    }
    frame_offs[n_utts] = f;
    return MCVC_OK;
}

int mcvc_audio_log_mel_launch(const float* wave, long long n_samples, const int* tiles, int n_tiles, const float* basis, float* out,
                              long long total_frames, hipStream_t s)
{
    if (!wave || !tiles || !basis || !out || n_samples < PAD + 1 || n_tiles < 1 || total_frames < 1) return MCVC_ERR_INVALID;
    if (((uintptr_t)wave & 3) || ((uintptr_t)out & 3) || ((uintptr_t)tiles & 15) || ((uintptr_t)basis & 15)) return MCVC_ERR_INVALID;
    static std::once_flag once;
    static hipError_t attr = hipSuccess;
    std::call_once(once, [] {
        attr = hipFuncSetAttribute(reinterpret_cast<const void*>(audio_log_mel_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_FLOATS * 4);
    });
    if (attr != hipSuccess) return (int)attr;
    AudioArgs a{wave, tiles, basis, out, n_samples, total_frames};
    const double fl = (double)n_tiles * TF * (2.0 * NFFT * NFFT + 4.0 * NBIN);
    TraceScope ts(K_SGEMM, s, fl, 4.0 * (n_samples + (double)NMEL * total_frames) + 4.0 * mcvc_audio_basis_floats_of());
    hipLaunchKernelGGL(audio_log_mel_kernel, dim3((unsigned)n_tiles), dim3(NTHREADS), LDS_FLOATS * 4, s, a);
    return (int)hipGetLastError();
}
