// Griffin-Lim decoder: log-mel [B][80][T] or linear magnitude [B][513][T] -> waveform [B][256 T], by phase reconstruction against the
// front-end's own STFT (audio_kernels.hip: reflect-pad 384, frames of 1024 at hop 256, periodic Hann, bins 0..512).  No weights.
//
//   M = max(0, pinv(mel basis) @ 10^logmel)                         (or the linear input itself)
//   ISTFT(S): frame_t = hann * irfft(S[:, t]);  y[p] = sum_t frame_t[p - 256 t] / sum_t hann^2[p - 256 t];  keep p in [384, 384 + 256 T)
//   A_0 given (unit modulus; NULL: zero phase), R_-1 = 0;  k = 0 .. n_iter - 1:
//       x = ISTFT(M A_k);  R_k = STFT(x);  Z = R_k - m / (1 + m) R_k-1;  A_k+1 = Z / |Z|  (0 where Z is 0)
//   out = ISTFT(M A_n)
//
// Three kernels plus the final overlap-add, 2 n_iter + 3 launches, no atomics anywhere: every value is a sum in one fixed order, so a
// sample's waveform does not depend on its batch or on anything else in the launch.
//
//   gl_init_kernel      the 513 x 80 pinv product (VALU, sequential fma over the 80 filters), clamp, times A_0 -> spectrum state
//   gl_inverse_kernel   spectrum state -> windowed frames.  A GEMM on v_mfma_f32_32x32x2_f32 per tile of 64 frames of one sample:
//                       M = sample in frame (1024, in two halves: a workgroup has 512 rows), N = frame (64), K = packed real spectrum
//                       (1024).  The inverse basis (hann[n] c_b cos / -sin (2 pi b n / 1024) / 1024, c_b = 1 for bins 0 and 512, else 2)
//                       streams from L2 to registers in lane order
//                       like the forward basis (stft.h: the same product); the spectrum tile (256 KB) does not fit LDS, so K runs in four chunks of 256 staged at
//                       257 floats per frame (conflict-free B reads).
//   gl_forward_kernel   windowed frames -> next spectrum state: the front-end's product with another loader and epilogue, literally --
//                       the tile, the reflected staging and the product are the code of stft.h that audio_log_mel_kernel runs, on the
//                       front-end's own operand.  The loader's sample is the sum of the at most 4 frame pieces that cover it, in
//                       ascending frame order, over the envelope; the epilogue has (re, im) of one (bin, frame) in one lane: momentum
//                       term from the stored R_k-1, normalise, times M, store M A_k+1 and R_k.
//   gl_overlap_add_kernel  the loader's overlap-add on its own, for the waveform.
//
// Packed spectrum of a frame ([1024] floats): (re, im) of bins 0..511 with the real part of bin 512 in the slot of bin 0's imaginary
// part -- the imaginary parts of bins 0 and 512 do not exist for a real signal and irfft ignores them.
//
// Workspace: spectrum [F][1024] | R [F][1024] | frames [F][1024] | M [F][514], F = B T.
#include "mcvc_common.h"
#include "griffinlim.h"
#include "stft.h"
#include "trace.h"

#include <cmath>
#include <mutex>
#include <vector>

namespace {

using namespace stft;

constexpr int KCHUNK = 256, CHUNK_LDS = TF * PITCH;        // inverse kernel: K staged 256 at a time, 257 floats per frame
static_assert(KCHUNK + 1 == PITCH && NFFT % KCHUNK == 0, "a chunk is staged at the pitch stft_product reads");
constexpr int MT_PER_WAVE = 2, M_SPLIT = 2;                // eight waves x two row tiles = half of the 32 row tiles; blockIdx.y has the half
constexpr int FLUSH_KG = 4;                                // k groups (32 terms) summed from zero before they join the running total (stft_product)
constexpr int MAG_LD = NBIN + 1;                           // M rows of 514: pairs of bins are 8-byte aligned
constexpr long long OFF_PINV = DFT_FLOATS, OFF_W2 = OFF_PINV + (long long)NBIN * NMEL, OFF_FWD = OFF_W2 + NFFT;
static_assert(OFF_W2 % 4 == 0 && OFF_FWD % 4 == 0, "16-byte aligned table sections");

struct GlArgs {
    const float* in;           // [B][80][T] or [B][513][T]
    const float* angles;       // [B][513][T][2] or null
    const float* tables;
    float* spec;               // [F][1024] packed M A_k
    float* prev;               // [F][1024] packed R_k-1
    float* frames;             // [F][1024] windowed frames
    float* mag;                // [F][514]
    float* out;                // [B][256 T]
    int B, T, kind, first;
    float coef;                // m / (1 + m)
};

// y[p] on the padded axis of one sample: frame pieces in ascending frame order over the window-square envelope (never zero in the kept range)
__device__ __forceinline__ float gl_ola(const float* __restrict__ fr, const float* __restrict__ w2, int T, int p)
{
    const int tlo = p < NFFT ? 0 : (p - (NFFT - HOP)) / HOP;
    int thi = p / HOP;
    if (thi > T - 1) thi = T - 1;
    float s = 0.f, e = 0.f;
    for (int t = tlo; t <= thi; ++t) {
        const int o = p - HOP * t;
        s += fr[(long long)t * NFFT + o];
        e += w2[o];
    }
    return s / e;
}

__global__ void __launch_bounds__(256) gl_init_kernel(const GlArgs a)
{
    __shared__ float e[NMEL][TF];
    const int tid = threadIdx.x, n = tid & 63, g = tid >> 6;
    const int b = blockIdx.y, t = blockIdx.x * TF + n, T = a.T;
    const bool valid = t < T;
    if (a.kind == MCVC_GL_KIND_LOGMEL) {
        for (int j = g; j < NMEL; j += 4) e[j][n] = valid ? exp10f(a.in[((long long)b * NMEL + j) * T + t]) : 0.f;
        __syncthreads();
    }
    const float* const pinv = a.tables + OFF_PINV;
    const long long f = (long long)b * T + t;
    for (int bin = g; bin < NBIN; bin += 4) {
        float m = 0.f;
        if (a.kind == MCVC_GL_KIND_LOGMEL) {
            for (int j = 0; j < NMEL; ++j) m = fmaf(pinv[bin * NMEL + j], e[j][n], m);
            m = fmaxf(m, 0.f);
        } else if (valid)
            m = a.in[((long long)b * NBIN + bin) * T + t];
        if (!valid) continue;
        float re = 1.f, im = 0.f;
        if (a.angles) {
            const float2 ang = reinterpret_cast<const float2*>(a.angles)[((long long)b * NBIN + bin) * T + t];
            re = ang.x; im = ang.y;
        }
        a.mag[f * MAG_LD + bin] = m;
        if (bin == 0) a.spec[f * NFFT] = m * re;
        else if (bin == NBIN - 1) a.spec[f * NFFT + 1] = m * re;
        else reinterpret_cast<float2*>(a.spec)[f * (NFFT / 2) + bin] = make_float2(m * re, m * im);
    }
}

__global__ void __launch_bounds__(NTHREADS) gl_inverse_kernel(const GlArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int T = a.T, tiles_per = (T + TF - 1) / TF;
    const int b = blockIdx.x / tiles_per, t0 = (blockIdx.x % tiles_per) * TF;
    if (b >= a.B) return;
    const int nv = T - t0 < TF ? T - t0 : TF;
    const long long f0 = (long long)b * T + t0;

    f32x16 acc[MT_PER_WAVE][2];
    stft_zero(acc);
    const int rt0 = (blockIdx.y * (NTHREADS / 64) + wave) * MT_PER_WAVE;     // the wave's first row tile
    const f32x4* const ap = reinterpret_cast<const f32x4*>(a.tables) + (long long)rt0 * KG * 64 + lane;
    const f32x4* const sp = reinterpret_cast<const f32x4*>(a.spec);
#pragma unroll 1
    for (int c = 0; c < NFFT / KCHUNK; ++c) {
        if (c) __syncthreads();                             // every wave is done with the previous chunk
        for (int i = tid; i < TF * (KCHUNK / 4); i += NTHREADS) {
            const int n = i >> 6, q = i & 63;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (n < nv) v = sp[(f0 + n) * (NFFT / 4) + c * (KCHUNK / 4) + q];
            float* d = smem + PITCH * n + 4 * q;
            d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
        }
        __syncthreads();
        stft_product<MT_PER_WAVE, FLUSH_KG, false>(acc, ap, stft_b_lane(smem, l31, half), c * (KCHUNK / 8), KCHUNK / 8);
    }
    // a basis row is a sample of the frame: row 2 p is sample 2 p
#pragma unroll
    for (int mt = 0; mt < MT_PER_WAVE; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int n = stft_col(l31, nt);
            if (n >= nv) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 v = {acc[mt][nt][4 * q], acc[mt][nt][4 * q + 1], acc[mt][nt][4 * q + 2], acc[mt][nt][4 * q + 3]};
                *reinterpret_cast<f32x4*>(a.frames + (f0 + n) * NFFT + 2 * stft_pair(rt0 + mt, q, half)) = v;
            }
        }
}

__device__ __forceinline__ float gl_sign(float z) { return z > 0.f ? 1.f : (z < 0.f ? -1.f : 0.f); }

__global__ void __launch_bounds__(NTHREADS) gl_forward_kernel(const GlArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int T = a.T, tiles_per = (T + TF - 1) / TF;
    const int b = blockIdx.x / tiles_per, t0 = (blockIdx.x % tiles_per) * TF;
    if (b >= a.B) return;
    const int nv = T - t0 < TF ? T - t0 : TF;
    const long long f0 = (long long)b * T + t0;

    // ---- the tile's samples: x = the overlap-add cropped to [384, 384 + 256 T), reflected at its own two ends ----
    const float* const fr = a.frames + (long long)b * T * NFFT;
    const float* const w2 = a.tables + OFF_W2;
    stft_stage_tile(smem, t0, nv, HOP * T, [&](int i) { return gl_ola(fr, w2, T, i + PAD); });

    f32x16 acc[MT_PER_WAVE][2];
    stft_zero(acc);
    const int rt0 = (blockIdx.y * (NTHREADS / 64) + wave) * MT_PER_WAVE;     // the wave's first row tile
    const f32x4* const ap = reinterpret_cast<const f32x4*>(a.tables + OFF_FWD) + (long long)rt0 * KG * 64 + lane;
    stft_product<MT_PER_WAVE, FLUSH_KG, true>(acc, ap, stft_b_lane(smem, l31, half), 0, KG);

    // ---- update: rows (2 pr, 2 pr + 1) of a lane are (sum x hann cos, sum x hann sin) = (Re, -Im) of one (bin, frame) ----
    const float c = a.coef;
    const f32x4* const pv4 = reinterpret_cast<const f32x4*>(a.prev);
    f32x4* const pw4 = reinterpret_cast<f32x4*>(a.prev);
    f32x4* const sp4 = reinterpret_cast<f32x4*>(a.spec);
#pragma unroll
    for (int mt = 0; mt < MT_PER_WAVE; ++mt) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int n = stft_col(l31, nt);
            if (n >= nv) continue;
            const long long f = f0 + n;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int bin = stft_pair(rt0 + mt, q, half);                         // this lane holds bins (bin, bin + 1)
                const long long at = f * (NFFT / 4) + (bin >> 1);
                f32x4 pv = {0.f, 0.f, 0.f, 0.f};
                if (!a.first) pv = pv4[at];
                const float2 m = *reinterpret_cast<const float2*>(a.mag + f * MAG_LD + bin);
                f32x4 r = {acc[mt][nt][4 * q], -acc[mt][nt][4 * q + 1], acc[mt][nt][4 * q + 2], -acc[mt][nt][4 * q + 3]};
                f32x4 o;
                if (bin == 0) {                             // (real DC, real Nyquist) share the pair
                    r[1] = -r[1];
                    o[0] = m.x * gl_sign(r[0] - c * pv[0]);
                    o[1] = a.mag[f * MAG_LD + NBIN - 1] * gl_sign(r[1] - c * pv[1]);
                } else {
                    const float zr = r[0] - c * pv[0], zi = r[1] - c * pv[1];
                    const float mod = sqrtf(zr * zr + zi * zi);
                    o[0] = mod > 0.f ? m.x * (zr / mod) : 0.f;
                    o[1] = mod > 0.f ? m.x * (zi / mod) : 0.f;
                }
                const float zr = r[2] - c * pv[2], zi = r[3] - c * pv[3];
                const float mod = sqrtf(zr * zr + zi * zi);
                o[2] = mod > 0.f ? m.y * (zr / mod) : 0.f;
                o[3] = mod > 0.f ? m.y * (zi / mod) : 0.f;
                sp4[at] = o;
                pw4[at] = r;
            }
        }
    }
}

__global__ void __launch_bounds__(256) gl_overlap_add_kernel(const GlArgs a)
{
    const int b = blockIdx.y, T = a.T, L = HOP * T;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= L) return;
    a.out[(long long)b * L + i] = gl_ola(a.frames + (long long)b * T * NFFT, a.tables + OFF_W2, T, i + PAD);
}

bool shape_ok(int B, int T)
{
    return B >= 1 && T >= MCVC_GL_MIN_FRAMES && T <= MCVC_GL_MAX_FRAMES && (long long)B * T <= (1LL << 22) && B <= 65535;
}

}  // namespace

int mcvc_gl_out_samples_of(int T) { return T < MCVC_GL_MIN_FRAMES || T > MCVC_GL_MAX_FRAMES ? 0 : HOP * T; }

int mcvc_gl_launches_of(int n_iter) { return n_iter < 0 ? 0 : 2 * n_iter + 3; }

long long mcvc_gl_tables_floats_of() { return OFF_FWD + mcvc_audio_basis_floats_of(); }

void mcvc_gl_tables_fill(const float* pinv, float* out)
{
    const Tables w;
    stft_fill_lane_order(out, [&](int k, int n) {           // IB[sample n][packed spectrum slot k]
        double v;
        if (k == 0) v = 1.0;                                // bin 0
        else if (k == 1) v = (n & 1) ? -1.0 : 1.0;          // bin 512: cos(pi n)
        else {
            const int ph = stft_phase(n, k >> 1);
            v = (k & 1) ? -2.0 * w.sn[ph] : 2.0 * w.cs[ph];
        }
        return w.hann[n] * v / NFFT;
    });
    for (int i = 0; i < NBIN * NMEL; ++i) out[OFF_PINV + i] = pinv[i];
    for (int k = 0; k < NFFT; ++k) out[OFF_W2 + k] = (float)(w.hann[k] * w.hann[k]);
    mcvc_audio_basis_fill(out + OFF_FWD);
}

long long mcvc_gl_workspace_floats_of(int B, int T)
{
    return shape_ok(B, T) ? (long long)B * T * (3 * NFFT + MAG_LD) : 0;
}

int mcvc_gl_decode_launch(const float* in, int in_kind, const float* angles0, const float* tables, float* out, float* ws, long long ws_floats,
                          int B, int T, int n_iter, float momentum, hipStream_t s)
{
    if (!in || !tables || !out || !shape_ok(B, T) || n_iter < 0 || !(momentum >= 0.f && momentum < 1.f)) return MCVC_ERR_INVALID;
    if (in_kind != MCVC_GL_KIND_LOGMEL && in_kind != MCVC_GL_KIND_LINEAR) return MCVC_ERR_INVALID;
    if (((uintptr_t)in & 3) || ((uintptr_t)angles0 & 7) || ((uintptr_t)tables & 15) || ((uintptr_t)out & 3) || ((uintptr_t)ws & 15)) return MCVC_ERR_INVALID;
    if (!ws || ws_floats < mcvc_gl_workspace_floats_of(B, T)) return MCVC_ERR_WORKSPACE;
    static std::once_flag once;
    static hipError_t attr = hipSuccess;
    std::call_once(once, [] {
        attr = hipFuncSetAttribute(reinterpret_cast<const void*>(gl_inverse_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, CHUNK_LDS * 4);
        if (attr == hipSuccess)
            attr = hipFuncSetAttribute(reinterpret_cast<const void*>(gl_forward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SPAN_LDS * 4);
    });
    if (attr != hipSuccess) return (int)attr;
    const long long F = (long long)B * T;
    GlArgs a{};
    a.in = in; a.angles = angles0; a.tables = tables; a.out = out;
    a.spec = ws; a.prev = ws + F * NFFT; a.frames = ws + 2 * F * NFFT; a.mag = ws + 3 * F * NFFT;
    a.B = B; a.T = T; a.kind = in_kind; a.first = 1; a.coef = momentum / (1.f + momentum);
    const int tiles_per = cdiv_i(T, TF);
    const unsigned n_tiles = (unsigned)(B * tiles_per);
    const double gemm_fl = (double)n_tiles * TF * 2.0 * NFFT * NFFT, state_b = 4.0 * F * NFFT, basis_b = 4.0 * DFT_FLOATS;
    hipError_t e;
    {
        TraceScope ts(K_ELEMENTWISE, s, in_kind == MCVC_GL_KIND_LOGMEL ? 2.0 * F * NBIN * NMEL : 0.0, 4.0 * F * (NFFT + 2 * NBIN));
        hipLaunchKernelGGL(gl_init_kernel, dim3((unsigned)tiles_per, (unsigned)B), dim3(256), 0, s, a);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    auto inverse = [&]() {
        TraceScope ts(K_SGEMM, s, gemm_fl, 2.0 * state_b + basis_b);
        hipLaunchKernelGGL(gl_inverse_kernel, dim3(n_tiles, M_SPLIT), dim3(NTHREADS), CHUNK_LDS * 4, s, a);
        return hipGetLastError();
    };
    for (int k = 0; k < n_iter; ++k) {
        if ((e = inverse()) != hipSuccess) return (int)e;
        a.first = k == 0;
        TraceScope ts(K_SGEMM, s, gemm_fl, 5.0 * state_b + basis_b);
        hipLaunchKernelGGL(gl_forward_kernel, dim3(n_tiles, M_SPLIT), dim3(NTHREADS), SPAN_LDS * 4, s, a);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    if ((e = inverse()) != hipSuccess) return (int)e;
    TraceScope ts(K_ELEMENTWISE, s, 8.0 * F * HOP, 4.0 * F * (NFFT + HOP));
    hipLaunchKernelGGL(gl_overlap_add_kernel, dim3((unsigned)cdiv_i(HOP * T, 256), (unsigned)B), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}
