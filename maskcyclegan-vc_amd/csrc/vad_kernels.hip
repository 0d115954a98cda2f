// Silence detection on a ragged bank of utterances: the frame energies librosa.effects.trim / split decide on (definition: include/mcvc.h;
// data_preprocessing/silence.py takes the decisions on the host; tests/silence_checker.py restates the energies in float64).
//
//   frame t of an utterance of L samples covers samples [512 t - 1024, 512 t + 1024), zero outside [0, L); T = 1 + L / 512 frames;
//   mse[t] = (1 / 2048) sum x^2;   ref = max_t mse[t].
//
//   vad_energy_kernel   one workgroup of 256 threads per ROW of mcvc_vad_plan's work list: up to 64 consecutive frames of one utterance.
//                       Frames overlap fourfold, so the workgroup first forms the sums of squares of the 512-sample BLOCKS
//                       [512 j, 512 j + 512) its frames touch (blocks t0 - 2 .. t0 + nv: nv + 3 of them) and keeps them in LDS, then a frame
//                       is the sum of its four blocks.  A sample is loaded once by the workgroup that owns it; the three blocks at a joint
//                       between two rows of one utterance are loaded by the neighbouring row as well (3 / 64 of a long utterance, from L2
//                       when the neighbours run together).
//   One summation order per frame, a function of the sample's index inside its own utterance alone: a block belongs to one wave; lane l
//   squares and adds samples 512 j + l + 64 i in the order i = 0 .. 7 (fused multiply-add: one rounding per term), so a wave-instruction
//   loads 256 consecutive bytes at any alignment of the bank (dword loads: nothing to peel, nothing that changes with the start offset);
//   the 64 partial sums are folded by a butterfly of fixed shape (xor 32, 16, .. 1); the frame is ((b0 + b1) + b2) + b3 in block order,
//   times 2^-11 (exact).  Samples outside [0, L) enter as zeros in the same places, never the neighbour's.
//   The maximum: a butterfly over the row's frames, then ONE integer atomic max per row on the value's bit pattern (energies are >= 0, so
//   the unsigned order is the float order): it has no order dependence.  mcvc_vad_energy zeroes ref with a memset node in front of the
//   kernel on the same stream: two launches.  No float atomic adds, no workspace, no device allocation.
//   LDS: nv + 3 <= 67 floats, all of it dynamic (base 16-byte aligned, no static in front of it); no scratch.
#include <climits>
#include <cstdint>

#include "mcvc_common.h"
#include "audio.h"
#include "trace.h"
#include "vad.h"

namespace {

constexpr int FRAME = MCVC_VAD_FRAME, HOP = MCVC_VAD_HOP, TF = MCVC_VAD_TILE_FRAMES;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int NBLK = TF + FRAME / HOP - 1;                   // blocks under TF consecutive frames
constexpr int LDS_FLOATS = (NBLK + 3) / 4 * 4;
static_assert(FRAME == 4 * HOP && HOP == 8 * 64, "a frame is four blocks; a lane owns eight samples of a block");
static_assert(TF >= 1 && TF <= 64, "one wave folds the row's maximum");

struct VadArgs {
    const float* wave;
    const int* tiles;          // [n_tiles][4] = first sample of the utterance, its length, utterance index, first frame of the row
    const int* frame_offs;     // [n_utts + 1]
    float* mse;                // [total_frames]
    float* ref;                // [n_utts], zeroed before the launch
    long long n_samples, total_frames;
    int n_utts;
};

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

__global__ __launch_bounds__(THREADS) void vad_energy_kernel(const VadArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float blk[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int4 row = reinterpret_cast<const int4*>(a.tiles)[blockIdx.x];
    const int s0 = row.x, L = row.y, u = row.z, t0 = row.w;
    // what the plan guarantees, once more (uniform: the whole workgroup leaves before its first barrier, nothing read or written)
    if (L < 1 || s0 < 0 || (long long)s0 + L > a.n_samples || u < 0 || u >= a.n_utts || t0 < 0 || t0 % TF != 0) return;
    const int T = 1 + L / HOP;
    if (t0 >= T) return;
    const long long fo = a.frame_offs[u];
    if (fo < 0 || fo + T > a.total_frames || a.frame_offs[u + 1] - fo != T) return;
    const int nv = T - t0 < TF ? T - t0 : TF;

    // ---- sums of squares of blocks t0 - 2 .. t0 + nv ----
    const float* const src = a.wave + s0;
    for (int jb = wave; jb < nv + 3; jb += WAVES) {
        const long long base = ((long long)t0 - 2 + jb) * HOP;          // (past 2^31 for the last blocks of the longest utterance)
        float acc = 0.f;
        if (base >= 0 && base < L) {
            const float* const p = src + base + lane;
            if (base + HOP <= L) {
                float x[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) x[i] = p[64 * i];
#pragma unroll
                for (int i = 0; i < 8; ++i) acc = fmaf(x[i], x[i], acc);
            } else {
                const int left = (int)(L - base) - lane;               // samples of the block at or after this lane's first
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float x = 64 * i < left ? p[64 * i] : 0.f;
                    acc = fmaf(x, x, acc);
                }
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) blk[jb] = acc;
    }
    __syncthreads();

    // ---- frames: block jb is block t0 - 2 + jb, frame t0 + i holds blocks jb = i .. i + 3 ----
    if (wave == 0) {
        float e = 0.f;
        if (lane < nv) {
            e = (((blk[lane] + blk[lane + 1]) + blk[lane + 2]) + blk[lane + 3]) * (1.0f / FRAME);
            a.mse[fo + t0 + lane] = e;
        }
        const float m = wave_max(e);
        if (lane == 0) atomicMax(reinterpret_cast<unsigned int*>(a.ref + u), __float_as_uint(m));
    }
}

}  // namespace

long long mcvc_vad_frames_of(long long n_samples) { return n_samples < 1 ? 0 : 1 + n_samples / HOP; }

int mcvc_vad_plan_host(const int* sample_offs, int n_utts, int* frame_offs, int* tiles, int max_tiles, int* n_tiles_out)
{
    if (!sample_offs || n_utts < 1 || !frame_offs || !n_tiles_out || sample_offs[0] < 0 || (tiles && max_tiles < 0)) return MCVC_ERR_INVALID;
    long long frames = 0, nt = 0;
    for (int u = 0; u < n_utts; ++u) {
        const long long L = (long long)sample_offs[u + 1] - sample_offs[u];
        if (L < 1) return MCVC_ERR_INVALID;                    // an empty utterance has no loudest frame
        const long long T = 1 + L / HOP;
        frames += T; nt += (T + TF - 1) / TF;
    }
    if (frames > INT_MAX || nt > INT_MAX) return MCVC_ERR_INVALID;     // (T <= L: cannot happen for int32 offsets)
    *n_tiles_out = (int)nt;
    int f = 0;
    long long k = 0;
    for (int u = 0; u < n_utts; ++u) {
        const int L = sample_offs[u + 1] - sample_offs[u], T = 1 + L / HOP;
        frame_offs[u] = f;
        for (int t0 = 0; tiles && t0 < T; t0 += TF, ++k)
            if (k < max_tiles) { int* const r = tiles + 4 * k; r[0] = sample_offs[u]; r[1] = L; r[2] = u; r[3] = t0; }
        f += T;
    }
    frame_offs[n_utts] = f;
    return tiles && nt > max_tiles ? MCVC_ERR_WORKSPACE : MCVC_OK;
}

int mcvc_audio_plan_segments_host(const int* starts, const int* lengths, int n_segs, int* frame_offs, int* tiles, int max_tiles, int* n_tiles_out)
{
    constexpr int ATF = MCVC_AUDIO_TILE_FRAMES;
    if (!starts || !lengths || n_segs < 1 || !frame_offs || !n_tiles_out || (tiles && max_tiles < 0)) return MCVC_ERR_INVALID;
    long long frames = 0, nt = 0;
    for (int u = 0; u < n_segs; ++u) {
        const long long L = lengths[u];
        if (starts[u] < 0 || L < MCVC_AUDIO_PAD + 1 || starts[u] + L > INT_MAX) return MCVC_ERR_INVALID;
        const long long T = (L - MCVC_AUDIO_HOP) / MCVC_AUDIO_HOP + 1;
        frames += T; nt += (T + ATF - 1) / ATF;
    }
    if (frames > INT_MAX) return MCVC_ERR_INVALID;
    *n_tiles_out = (int)nt;
    if (tiles && nt > max_tiles) return MCVC_ERR_WORKSPACE;
    int f = 0, k = 0;
    for (int u = 0; u < n_segs; ++u) {
        const int L = lengths[u], T = mcvc_audio_frames_of(L);
        frame_offs[u] = f;
        for (int t0 = 0; tiles && t0 < T; t0 += ATF, ++k) {
            tiles[4 * k] = starts[u]; tiles[4 * k + 1] = L; tiles[4 * k + 2] = f + t0; tiles[4 * k + 3] = t0;
        }
        f += T;
    }
    frame_offs[n_segs] = f;
    return MCVC_OK;
}

int mcvc_vad_energy_launch(const float* wave, long long n_samples, const int* tiles, int n_tiles, const int* frame_offs_dev, int n_utts, float* mse,
                           long long total_frames, float* ref, hipStream_t s)
{
    if (!wave || !tiles || !frame_offs_dev || !mse || !ref || n_samples < 1 || n_samples > INT_MAX || n_tiles < 1 || n_utts < 1 || total_frames < 1 ||
        total_frames > INT_MAX)
        return MCVC_ERR_INVALID;
    if (((uintptr_t)wave & 3) || ((uintptr_t)mse & 3) || ((uintptr_t)ref & 3) || ((uintptr_t)frame_offs_dev & 3) || ((uintptr_t)tiles & 15))
        return MCVC_ERR_INVALID;
    const hipError_t z = hipMemsetAsync(ref, 0, sizeof(float) * (size_t)n_utts, s);
    if (z != hipSuccess) return (int)z;
    const VadArgs a{wave, tiles, frame_offs_dev, mse, ref, n_samples, total_frames, n_utts};
    TraceScope ts(K_ELEMENTWISE, s, 2.0 * (double)n_samples, 4.0 * ((double)n_samples + (double)total_frames + (double)n_utts));
    hipLaunchKernelGGL(vad_energy_kernel, dim3((unsigned)n_tiles), dim3(THREADS), LDS_FLOATS * 4, s, a);
    return (int)hipGetLastError();
}
