// MelGAN decoder (log-mel -> waveform), fp32, inference only: the second half of the vocoder whose first half is audio_kernels.hip.
// The reference obtains it through torch.hub (mask_cyclegan_vc/test.py:94-103, utils.py:25-39: vocoder.inverse); this file restates
// Generator(input_size 80, ngf 32, n_residual_layers 3) of Kumar et al. 2019 from its published definition:
//
//   reflect 3 | Conv1d(80, 512, 7) | 4 x [ LeakyReLU(0.2) | ConvTranspose1d(C, C/2, 2r, stride r) | 3 x ResnetBlock(C/2, dilation 1, 3, 9) ]
//   with r = 8, 8, 2, 2 | LeakyReLU | reflect 3 | Conv1d(32, 1, 7) | tanh ;
//   ResnetBlock(x) = shortcut(x) + conv1x1(lrelu(conv3_d(reflect_d(lrelu(x))))).
//
// Every layer but the last is one implicit GEMM on v_mfma_f32_32x32x2_f32 (voc_gemm_kernel): M = output row, N = time, K = (input channel,
// tap).  Activations stay [B][C][L] with time contiguous.  A workgroup owns BM rows x BN time steps of one sample; per chunk of 16 or 32
// input channels it stages the time span its taps reach (BN + (taps - 1) * dilation floats per channel) in LDS ONCE -- reflection at the
// row's own two ends is index arithmetic at that point (the edge sample is not repeated), LeakyReLU is applied on the way in -- and every
// tap reads a shifted window of it.  No im2col buffer, no padded copy, no stand-alone elementwise launch.
//
//   VOC_CONV    taps = k, window shift tap * d - (k - 1) d / 2, reflection.
//   VOC_CONVT   k = 2r, stride r, padding r / 2: output t = r q + ph reads input q (weight tap ph + r/2) and one neighbour: q - 1 (tap
//               ph + r/2 + r) when ph < r/2, else q + 1 (tap ph - r/2).  So the rows are two GROUPS, each a 2-tap convolution with zero
//               padding over Cout * r/2 rows: group g has phases g r/2 .. g r/2 + r/2 - 1 and window shifts {g - 1, g}.  Row
//               g * Mg + co * r/2 + p is (channel co, phase g r/2 + p): the four accumulator registers a lane holds for four consecutive
//               rows are four consecutive output samples (r = 8: one 16-byte store).  No scatter, no atomics, no inserted zeros.
//   VOC_STACK   the two 1 x 1 products of a ResnetBlock share their output: K runs over [x ; lrelu(h)], 2 dim channels, so the residual
//               sum is the GEMM's own accumulation.  A block is two launches, a decode 1 + 4 * (1 + 3 * 2) + 1 = 30.
//   VOC_LAST    Conv1d(32, 1, 7) + tanh has one output row: voc_last_kernel, one thread per sample on the vector ALU.
//
// Packed weights (mcvc_voc_pack, HOST, once per checkpoint; weight norm is folded by the caller in float64).  K order is (chunk of CC
// channels, tap, channel in chunk), CC = 32 (16 when the channel count is no multiple of 32: the 80 mel rows).  Like the DFT basis of
// audio_kernels.hip the operand goes from L2 straight to registers in the order the lanes consume it:
// float index ((mt * KG + kg) * 64 + lane) * 4 + j  =  W[row 32 mt + (lane & 31)][k = 8 kg + 2 j + (lane >> 5)], one 16-byte load per
// lane, row tile and eight k, fetched one k group ahead.  The rows' biases follow (VOC_STACK: the sum of the two).
//
// Rounding.  An MFMA chain is a k-ordered fmaf chain.  Each chunk (32 x taps terms at most) is summed from zero in accumulators of its
// own and then added to the running total, so no chain is longer than 224 + 32 terms whatever K is (wino_gemm's two levels).  One
// accumulation order, no atomics: two runs are bit-equal and a sample's result does not depend on the batch it is in.
#include "mcvc_common.h"
#include "vocoder.h"
#include "trace.h"

#include <mutex>
#include <vector>

namespace {

constexpr int NTHREADS = 256;

struct VocGemmArgs {
    const float* x0;           // [B][C0][L]
    const float* x1;           // [B][C1][L] (VOC_STACK), else unused
    const float* w;            // packed rows, lane order
    const float* bias;         // [Mtot]
    float* y;                  // [B][Cout][Lout]
    long long Lout;
    int C0, C1, act0, act1;    // act: LeakyReLU(0.2) while staging
    int L;                     // input length = the GEMM's N
    int taps, dil, pad;        // window of tap k starts at t + k * dil - pad (group g of a transposed conv: pad - g)
    int reflect;               // 1 reflection, 0 zeros beyond the ends
    int cc_log2, nchunks;      // channels per chunk (16 / 32), chunks over C0 + C1
    int Mg, Mtot;              // rows per group, rows in all
    int ph_log2, r;            // rows per output channel (phases of a group), output stride
    int Cout;
    int span;                  // floats staged per channel = BN + (taps - 1) * dil
};

template <int WM, int TM>
__global__ void __launch_bounds__(NTHREADS) voc_gemm_kernel(const VocGemmArgs a)
{
    constexpr int WN = 4 / WM, TN = 4 / TM, BM = 32 * WM * TM, BN = 32 * WN * TN;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM, b = blockIdx.z;
    if (n0 >= a.L || m0 + BM > a.Mtot) return;              // a tile outside the problem is skipped (workgroup-uniform, before any barrier)
    const int grp = m0 >= a.Mg ? 1 : 0;
    const int pad = a.pad - grp;
    const int CC = 1 << a.cc_log2, cc8 = CC >> 3;
    const int kgs = a.taps * cc8;                           // k groups of 8 per chunk
    const int KG = a.nchunks * kgs;
    const f32x4* const ap = reinterpret_cast<const f32x4*>(a.w) + (long long)((m0 >> 5) + wm * TM) * KG * 64 + lane;

    f32x16 acc[TM][TN], part[TM][TN];
#pragma unroll
    for (int mt = 0; mt < TM; ++mt)
#pragma unroll
        for (int nt = 0; nt < TN; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.f;

    f32x4 cur[TM], nxt[TM];
#pragma unroll
    for (int mt = 0; mt < TM; ++mt) cur[mt] = ap[(long long)mt * KG * 64];

    const float* const b_lane = smem + half * a.span + wn * (TN * 32) + l31;

#pragma unroll 1
    for (int chunk = 0; chunk < a.nchunks; ++chunk) {
        // ---- stage CC channels x span samples: reflection / zeros at the row's own ends, LeakyReLU on the way in ----
        const int ch0 = chunk << a.cc_log2;
        const bool seg1 = ch0 >= a.C0;
        const float* const xs = seg1 ? a.x1 + ((long long)b * a.C1 + (ch0 - a.C0)) * a.L : a.x0 + ((long long)b * a.C0 + ch0) * a.L;
        const int act = seg1 ? a.act1 : a.act0;
        __syncthreads();                                    // every wave is done reading the previous chunk
        for (int c = wave; c < CC; c += NTHREADS / 64) {
            const float* const row = xs + (long long)c * a.L;
            float* const dst = smem + c * a.span;
            for (int s = lane; s < a.span; s += 64) {
                int i = n0 - pad + s;
                if (a.reflect) {
                    if (i < 0) i = -i;
                    if (i >= a.L) i = 2 * (a.L - 1) - i;
                }
                float v = 0.f;
                if (i >= 0 && i < a.L) v = row[i];          // (columns at or beyond L are staged as zeros and never stored)
                if (act) v = v > 0.f ? v : 0.2f * v;
                dst[s] = v;
            }
        }
        __syncthreads();

#pragma unroll
        for (int mt = 0; mt < TM; ++mt)
#pragma unroll
            for (int nt = 0; nt < TN; ++nt)
#pragma unroll
                for (int i = 0; i < 16; ++i) part[mt][nt][i] = 0.f;

#pragma unroll 1
        for (int g = 0; g < kgs; ++g) {
            const int kgg = chunk * kgs + g;
            const int kn = kgg + 1 < KG ? kgg + 1 : kgg;    // (the last fetch is a repeat nobody uses)
#pragma unroll
            for (int mt = 0; mt < TM; ++mt) nxt[mt] = ap[((long long)mt * KG + kn) * 64];
            const int tap = g >> (a.cc_log2 - 3), kg8 = g & (cc8 - 1);
            const float* const bp = b_lane + (8 * kg8) * a.span + tap * a.dil;   // k = 8 kg8 + 2 j + half: channel row, window shift tap * dil
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float bv[TN];
#pragma unroll
                for (int nt = 0; nt < TN; ++nt) bv[nt] = bp[(2 * j) * a.span + 32 * nt];
#pragma unroll
                for (int mt = 0; mt < TM; ++mt)
#pragma unroll
                    for (int nt = 0; nt < TN; ++nt)
                        part[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[mt][j], bv[nt], part[mt][nt], 0, 0, 0);
            }
#pragma unroll
            for (int mt = 0; mt < TM; ++mt) cur[mt] = nxt[mt];
        }
#pragma unroll
        for (int mt = 0; mt < TM; ++mt)
#pragma unroll
            for (int nt = 0; nt < TN; ++nt) acc[mt][nt] += part[mt][nt];
    }

    // ---- bias, store: accumulator register 4 q + i of a lane is row 8 q + 4 half + i, column lane & 31 of its tile ----
    const int PH = 1 << a.ph_log2;
#pragma unroll
    for (int mt = 0; mt < TM; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = m0 + 32 * (wm * TM + mt) + 8 * q + 4 * half;          // (a multiple of 4)
            const f32x4 bs = *reinterpret_cast<const f32x4*>(a.bias + row);
            const int ml = row - grp * a.Mg;
#pragma unroll
            for (int nt = 0; nt < TN; ++nt) {
                const int col = n0 + 32 * (wn * TN + nt) + l31;
                if (col >= a.L) continue;
                const long long t0 = (long long)col * a.r + grp * PH;
                if (a.ph_log2 == 2) {                       // four phases of one channel: four consecutive samples
                    f32x4 v;
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = acc[mt][nt][4 * q + i] + bs[i];
                    *reinterpret_cast<f32x4*>(a.y + ((long long)b * a.Cout + (ml >> 2)) * a.Lout + t0) = v;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int m = ml + i;
                        a.y[((long long)b * a.Cout + (m >> a.ph_log2)) * a.Lout + t0 + (m & (PH - 1))] = acc[mt][nt][4 * q + i] + bs[i];
                    }
                }
            }
        }
}

struct VocLastArgs {
    const float* x;            // [B][C][L]
    const float* w;            // [C][k] then the bias
    float* y;                  // [B][L]
    int C, L, k;
};

// y[b][t] = tanh(bias + sum_{c, j} w[c][j] * lrelu(x[b][c][refl(t + j - (k - 1) / 2)])): one output row, so no matrix tile (31 of its 32 rows
// would be padding).  The weights are wave-uniform loads; each channel's taps are summed on their own and then added to the total.
__global__ void __launch_bounds__(NTHREADS) voc_last_kernel(const VocLastArgs a)
{
    const long long t_ll = (long long)blockIdx.x * NTHREADS + threadIdx.x;
    if (t_ll >= a.L) return;
    const int t = (int)t_ll, b = blockIdx.y, pad = (a.k - 1) / 2;
    const float* row = a.x + (long long)b * a.C * a.L;
    float acc = 0.f;
    for (int c = 0; c < a.C; ++c, row += a.L) {
        float p = 0.f;
        for (int j = 0; j < a.k; ++j) {
            int i = t + j - pad;
            if (i < 0) i = -i;
            if (i >= a.L) i = 2 * (a.L - 1) - i;
            float v = (i >= 0 && i < a.L) ? row[i] : 0.f;
            v = v > 0.f ? v : 0.2f * v;
            p = fmaf(a.w[c * a.k + j], v, p);
        }
        acc += p;
    }
    a.y[(long long)b * a.L + t] = tanhf(acc + a.w[a.C * a.k]);
}

// ---- host ----
inline long long round4(long long n) { return (n + 3) & ~3LL; }
inline int cc_of(int ctot) { return ctot % 32 == 0 ? 32 : 16; }
inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
inline int log2i(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// the GEMM view of a layer: rows, K channels, taps
struct VocShape { int Mg, Mtot, Ctot, taps, PH; };

bool shape_of(int kind, int Cin, int Cout, int k, int r, VocShape* sh)
{
    if (Cin < 1 || Cout < 1) return false;
    switch (kind) {
    case VOC_CONV:
        if (Cout % 32 || Cin % 16 || k < 1 || !(k & 1) || k > 15) return false;
        *sh = VocShape{Cout, Cout, Cin, k, 1};
        return true;
    case VOC_CONVT:
        if (r < 2 || (r & 1) || !pow2(r / 2) || r > 16 || k != 2 * r || Cin % 16 || (Cout * (r / 2)) % 32) return false;
        *sh = VocShape{Cout * (r / 2), Cout * r, Cin, 2, r / 2};
        return true;
    case VOC_STACK:
        if (Cin != Cout || Cout % 32 || k != 1) return false;
        *sh = VocShape{Cout, Cout, 2 * Cout, 1, 1};
        return true;
    default:
        return false;
    }
}

template <int WM, int TM>
int launch_cfg(const VocGemmArgs& a0, int B, hipStream_t s)
{
    constexpr int BM = 32 * WM * TM, BN = 32 * (4 / WM) * (4 / TM);
    VocGemmArgs a = a0;
    a.span = BN + (a.taps - 1) * a.dil;
    const size_t lds = (size_t)(1 << a.cc_log2) * a.span * 4;
    static std::once_flag once;
    static hipError_t attr = hipSuccess;
    std::call_once(once, [] {
        attr = hipFuncSetAttribute(reinterpret_cast<const void*>(voc_gemm_kernel<WM, TM>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    });
    if (attr != hipSuccess) return (int)attr;
    if (lds > 96 * 1024) return MCVC_ERR_INVALID;
    const long long nt = cdiv_ll(a.L, BN);
    if (nt > 0x7fffffffLL || a.Mtot / BM > 65535 || B > 65535) return MCVC_ERR_INVALID;
    hipLaunchKernelGGL((voc_gemm_kernel<WM, TM>), dim3((unsigned)nt, (unsigned)(a.Mtot / BM), (unsigned)B), dim3(NTHREADS), lds, s, a);
    return (int)hipGetLastError();
}

}  // namespace

long long mcvc_voc_layer_packed_floats_of(int kind, int Cin, int Cout, int k, int r)
{
    if (kind == VOC_LAST) return (Cout == 1 && Cin >= 1 && k >= 1 && (k & 1) && k <= 15) ? round4((long long)Cin * k + 1) : 0;
    VocShape sh;
    if (!shape_of(kind, Cin, Cout, k, r, &sh)) return 0;
    return round4((long long)sh.Mtot * sh.Ctot * sh.taps) + round4(sh.Mtot);
}

int mcvc_voc_layer_pack_host(int kind, const float* w0, const float* b0, const float* w1, const float* b1, float* packed, int Cin, int Cout, int k, int r)
{
    if (!w0 || !b0 || !packed || mcvc_voc_layer_packed_floats_of(kind, Cin, Cout, k, r) == 0) return MCVC_ERR_INVALID;
    if (kind == VOC_LAST) {
        for (int i = 0; i < Cin * k; ++i) packed[i] = w0[i];
        packed[Cin * k] = b0[0];
        for (long long i = (long long)Cin * k + 1; i < round4((long long)Cin * k + 1); ++i) packed[i] = 0.f;
        return MCVC_OK;
    }
    if (kind == VOC_STACK && (!w1 || !b1)) return MCVC_ERR_INVALID;
    VocShape sh;
    shape_of(kind, Cin, Cout, k, r, &sh);
    const int CC = cc_of(sh.Ctot), per_chunk = sh.taps * CC, KG = sh.Ctot * sh.taps / 8;
    for (int mt = 0; mt < sh.Mtot / 32; ++mt)
        for (int kg = 0; kg < KG; ++kg)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int m = 32 * mt + (lane & 31), kl = 8 * kg + 2 * j + (lane >> 5);
                    const int chunk = kl / per_chunk, tap = (kl % per_chunk) / CC, ch = chunk * CC + kl % CC;
                    float v;
                    if (kind == VOC_CONV)
                        v = w0[((long long)m * Cin + ch) * k + tap];
                    else if (kind == VOC_CONVT) {               // torch layout [Cin][Cout][2r]; group g, window shift tap - 1 + g
                        const int g = m / sh.Mg, ml = m % sh.Mg, co = ml / sh.PH, ph = g * sh.PH + ml % sh.PH;
                        v = w0[((long long)ch * Cout + co) * k + r * (1 - tap - g) + ph + r / 2];
                    } else
                        v = ch < Cout ? w0[(long long)m * Cout + ch] : w1[(long long)m * Cout + ch - Cout];
                    packed[(((long long)mt * KG + kg) * 64 + lane) * 4 + j] = v;
                }
    float* bias = packed + round4((long long)sh.Mtot * sh.Ctot * sh.taps);
    for (int m = 0; m < sh.Mtot; ++m) {
        if (kind == VOC_CONVT) bias[m] = b0[(m % sh.Mg) / sh.PH];
        else if (kind == VOC_STACK) bias[m] = b0[m] + b1[m];
        else bias[m] = b0[m];
    }
    return MCVC_OK;
}

int mcvc_voc_layer_launch(int kind, const float* packed, const float* x0, const float* x1, float* y, int B, int Cin, int Cout, int L, int k, int dil, int r,
                          int act_in, hipStream_t s)
{
    if (!packed || !x0 || !y || B < 1 || L < 1 || mcvc_voc_layer_packed_floats_of(kind, Cin, Cout, k, r) == 0) return MCVC_ERR_INVALID;
    if (((uintptr_t)packed & 15) || ((uintptr_t)y & 15) || ((uintptr_t)x0 & 3) || ((uintptr_t)x1 & 3)) return MCVC_ERR_INVALID;
    if (kind == VOC_LAST) {
        if ((k - 1) / 2 > L - 1 || B > 65535) return MCVC_ERR_INVALID;      // reflection needs more samples than it adds
        VocLastArgs a{x0, packed, y, Cin, L, k};
        TraceScope ts(K_ELEMENTWISE, s, 2.0 * B * Cin * k * L, 4.0 * B * (Cin + 1.0) * L);
        hipLaunchKernelGGL(voc_last_kernel, dim3((unsigned)cdiv_i(L, NTHREADS), (unsigned)B), dim3(NTHREADS), 0, s, a);
        return (int)hipGetLastError();
    }
    VocShape sh;
    shape_of(kind, Cin, Cout, k, r, &sh);
    if (kind == VOC_STACK && !x1) return MCVC_ERR_INVALID;
    if (kind != VOC_CONVT) r = 1;
    if (kind != VOC_CONV) dil = 1;
    if (dil < 1 || dil > 64) return MCVC_ERR_INVALID;
    const int pad = kind == VOC_CONV ? (k - 1) * dil / 2 : kind == VOC_CONVT ? 1 : 0;
    if (kind == VOC_CONV && pad > L - 1) return MCVC_ERR_INVALID;
    if ((long long)L * r > 0x7fffffffLL) return MCVC_ERR_INVALID;
    VocGemmArgs a{};
    a.x0 = x0; a.x1 = kind == VOC_STACK ? x1 : x0;
    a.w = packed; a.bias = packed + round4((long long)sh.Mtot * sh.Ctot * sh.taps); a.y = y;
    a.Lout = (long long)L * r;
    a.C0 = kind == VOC_STACK ? Cout : Cin; a.C1 = kind == VOC_STACK ? Cout : 0;
    a.act0 = kind == VOC_STACK ? 0 : (act_in ? 1 : 0); a.act1 = 1;
    a.L = L; a.taps = sh.taps; a.dil = dil; a.pad = pad; a.reflect = kind == VOC_CONVT ? 0 : 1;
    a.cc_log2 = cc_of(sh.Ctot) == 32 ? 5 : 4; a.nchunks = sh.Ctot >> a.cc_log2;
    a.Mg = sh.Mg; a.Mtot = sh.Mtot; a.ph_log2 = log2i(sh.PH); a.r = r; a.Cout = Cout;
    TraceScope ts(K_SGEMM, s, 2.0 * B * sh.Mtot * sh.Ctot * sh.taps * L, 4.0 * B * ((double)sh.Ctot + sh.Mtot) * L + 4.0 * sh.Mtot * sh.Ctot * sh.taps);
    if (sh.Mg % 128 == 0) return launch_cfg<2, 2>(a, B, s);        // 128 rows x 128 samples
    if (sh.Mg % 64 == 0) return launch_cfg<1, 2>(a, B, s);         //  64 rows x 256 samples
    return launch_cfg<1, 1>(a, B, s);                              //  32 rows x 512 samples: one row tile, time is the wide side
}

// ---- the whole decoder ----
namespace {

struct VocOp { int kind, Cin, Cout, k, dil, r, act, l0, l1; long long off; };

const std::vector<VocOp>& voc_ops()
{
    static std::vector<VocOp> ops;
    static std::once_flag once;
    std::call_once(once, [] {
        // layers in state-dict order: 0 = model.1; stage s: 1 + 10 s = the transposed conv, then per block (block.2, block.4, shortcut); 41 = model.24
        ops.push_back(VocOp{VOC_CONV, MCVC_VOC_NMEL, 512, 7, 1, 1, 0, 0, -1, 0});
        const int rs[4] = {8, 8, 2, 2};
        for (int st = 0; st < 4; ++st) {
            const int Cin = 512 >> st, C = Cin / 2, base = 1 + 10 * st;
            ops.push_back(VocOp{VOC_CONVT, Cin, C, 2 * rs[st], 1, rs[st], 1, base, -1, 0});
            for (int j = 0, d = 1; j < 3; ++j, d *= 3) {
                ops.push_back(VocOp{VOC_CONV, C, C, 3, d, 1, 1, base + 1 + 3 * j, -1, 0});
                ops.push_back(VocOp{VOC_STACK, C, C, 1, 1, 1, 0, base + 3 + 3 * j, base + 2 + 3 * j, 0});
            }
        }
        ops.push_back(VocOp{VOC_LAST, 32, 1, 7, 1, 1, 1, MCVC_VOC_NLAYERS - 1, -1, 0});
        long long off = 0;
        for (VocOp& o : ops) { o.off = off; off += mcvc_voc_layer_packed_floats_of(o.kind, o.Cin, o.Cout, o.k, o.r); }
    });
    return ops;
}

constexpr long long VOC_BUF_PER_FRAME = 8192;               // the widest activation: 128 x 64 T = 64 x 128 T = 32 x 256 T floats per sample

}  // namespace

long long mcvc_voc_packed_floats_of()
{
    const VocOp& o = voc_ops().back();
    return o.off + mcvc_voc_layer_packed_floats_of(o.kind, o.Cin, o.Cout, o.k, o.r);
}

int mcvc_voc_pack_host(const float* const* table, float* packed)
{
    if (!table || !packed) return MCVC_ERR_INVALID;
    for (int i = 0; i < 2 * MCVC_VOC_NLAYERS; ++i)
        if (!table[i]) return MCVC_ERR_INVALID;
    for (const VocOp& o : voc_ops()) {
        const float* w1 = o.l1 >= 0 ? table[2 * o.l1] : nullptr;
        const float* b1 = o.l1 >= 0 ? table[2 * o.l1 + 1] : nullptr;
        const int rc = mcvc_voc_layer_pack_host(o.kind, table[2 * o.l0], table[2 * o.l0 + 1], w1, b1, packed + o.off, o.Cin, o.Cout, o.k, o.r);
        if (rc != MCVC_OK) return rc;
    }
    return MCVC_OK;
}

long long mcvc_voc_workspace_floats_of(int B, int T)
{
    if (B < 1 || T < MCVC_VOC_MIN_FRAMES) return 0;
    return 3 * VOC_BUF_PER_FRAME * B * T;                   // block input, the block's 3-tap product, block output; rotated
}

int mcvc_voc_decode_launch(const float* packed, const float* mel, float* out, float* ws, long long ws_floats, int B, int T, hipStream_t s)
{
    if (!packed || !mel || !out || B < 1 || B > 65535 || T < MCVC_VOC_MIN_FRAMES || T > (1 << 20)) return MCVC_ERR_INVALID;
    if (!ws || ws_floats < mcvc_voc_workspace_floats_of(B, T)) return MCVC_ERR_WORKSPACE;
    if (((uintptr_t)packed & 15) || ((uintptr_t)ws & 15) || ((uintptr_t)mel & 3) || ((uintptr_t)out & 15)) return MCVC_ERR_INVALID;
    float* buf[3];
    for (int i = 0; i < 3; ++i) buf[i] = ws + i * VOC_BUF_PER_FRAME * B * T;
    const float* x = mel;
    int cur = 2, L = T;                                     // (the first layer writes buf[0])
    for (const VocOp& o : voc_ops()) {
        const float* w = packed + o.off;
        int rc;
        if (o.kind == VOC_LAST)
            rc = mcvc_voc_layer_launch(o.kind, w, x, nullptr, out, B, o.Cin, o.Cout, L, o.k, o.dil, o.r, o.act, s);
        else if (o.kind == VOC_CONV && o.k == 3) {          // a block's first half: h is read by the VOC_STACK launch that follows
            rc = mcvc_voc_layer_launch(o.kind, w, x, nullptr, buf[(cur + 2) % 3], B, o.Cin, o.Cout, L, o.k, o.dil, o.r, o.act, s);
        } else {
            const int nx = (cur + 1) % 3;
            rc = mcvc_voc_layer_launch(o.kind, w, x, buf[(cur + 2) % 3], buf[nx], B, o.Cin, o.Cout, L, o.k, o.dil, o.r, o.act, s);
            cur = nx; x = buf[cur]; L *= o.r;
        }
        if (rc != MCVC_OK) return rc;
    }
    return MCVC_OK;
}
