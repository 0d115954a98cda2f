// Mel inversion by non-negative least squares: log-mel [B][80][T] -> linear magnitude [B][513][T], the input mcvc_gl_decode takes as
// MCVC_GL_KIND_LINEAR.  min_{M >= 0} || Bm M - y ||^2, y = 10^logmel, Bm the [80][513] Slaney basis, by a fixed number of FISTA steps from
// the decoder's own start value -- the problem is underdetermined (80 equations, 513 unknowns), so the result IS this iteration:
//
//   M_0 = max(0, P y)  (gl_init_kernel's arithmetic: exp10f, one fmaf chain over filters 0..79 from zero),  Z_0 = M_0
//   k < n_iter:  r = Bm Z_k - y;  M_k+1 = max(0, Z_k - s Bm^T r);  Z_k+1 = M_k+1 + beta_k (M_k+1 - M_k)
//   s = 1 / lambda_max(Bm Bm^T),  beta_k = (t_k - 1) / t_k+1,  t_0 = 1,  t_k+1 = (1 + sqrt(1 + 4 t_k^2)) / 2  (float64 on the host, used as float32)
//
// One launch whatever n_iter is.  A workgroup owns TF consecutive frames of one sample for the whole iteration; the frame is the fast
// index of every LDS row and of both global layouts.  Thread (g, n) = (tid / TF, tid % TF) owns bins g, g + 16, g + 32, ... of frame n:
// their M and Z never leave its registers (33 of each per thread); what other threads read -- Z for the filter sums -- is published to
// LDS as float32, beside y, r and the tables.
//
// Precision.  Both products are float32 in the one order given below.  The STATE is carried in float64 by its owner: the update
// M' = max(0, Z - s g), Z' = M' + beta (M' - M) is exact to 2^-53, and M is rounded to float32 once, at the store.  Why: B^T r lies in
// the row space of B, so the iteration corrects an error there but never one in the 433-dimensional null space; with a float32 state the
// update's own rounding walks off along it (1e-6 of the frame maximum after 16 steps, 3e-5 after 128), with this one it does not
// (DESIGN.md "Mel inversion" has the figures).  n_iter = 0 is untouched by this: float(double(M_0)) = M_0.
//
// The basis is never multiplied densely.  A bin's column has at most two non-zeros, in adjacent filters; a filter's non-zeros are
// contiguous bins (at most 41 of them).  mcvc_melinv_tables_fill checks exactly that and refuses anything else.
//   phase A  r_j = (sum over the filter's bins, ascending, one fmaf chain from zero) - y_j      16 groups x 5 rounds = 80 filters; odd
//            rounds run the groups in reverse so the long high filters meet the short ends of the round before
//   phase B  g = fmaf(w1, r_f+1, w0 r_f) in float32;  M' = max(0, fma(-s, g, Z));  Z = fma(beta, M' - M, M') in float64, per owned bin; a bin
//            in no filter (0 and 512) keeps its start value
// No atomics, one order per sum, nothing shared between frames: a frame's result does not depend on its batch, its position or T.
#include "mcvc_common.h"
#include "griffinlim.h"
#include "melinv.h"
#include "trace.h"

#include <cmath>
#include <mutex>

namespace {

constexpr int NBIN = 513, NMEL = 80, NBIN_LD = 516;        // table rows of 516: 16-byte aligned sections
constexpr int GROUPS = 16, ROUNDS = NMEL / GROUPS;         // threads of a workgroup: 16 groups of TF frames (256)
constexpr int CHUNK = 8;                                   // filter terms whose LDS reads are issued together
constexpr int FW_LD = 1028;                                // at most 2 x 513 non-zeros
static_assert(NMEL % GROUPS == 0, "every group has a filter in every round");
constexpr long long OFF_PINV = 0, OFF_STEP = OFF_PINV + (long long)NBIN * NMEL, OFF_BETA = OFF_STEP + 4, OFF_CST = OFF_BETA + MCVC_MELINV_MAX_ITER;
// the section a workgroup copies to LDS, offsets inside it
constexpr int C_BINF = 0, C_W0 = C_BINF + NBIN_LD, C_W1 = C_W0 + NBIN_LD, C_FILT = C_W1 + NBIN_LD, C_FW = C_FILT + 4 * NMEL, CST_FLOATS = C_FW + FW_LD;
constexpr long long TABLE_FLOATS = OFF_CST + CST_FLOATS;
static_assert(OFF_STEP % 4 == 0 && OFF_CST % 4 == 0 && C_FILT % 4 == 0 && C_FW % 4 == 0 && CST_FLOATS % 4 == 0, "16-byte aligned table sections");

struct MelinvArgs {
    const float* in;           // [B][80][T]
    const float* tables;
    float* out;                // [B][513][T]
    int B, T, n_iter;
};

constexpr int TF = 16;                                     // frames of a workgroup: DESIGN.md "Mel inversion" has the measurement against 32
constexpr int LDS_FLOATS = (NBIN + 2 * NMEL) * TF + CST_FLOATS;

__global__ void __launch_bounds__(GROUPS * TF) melinv_kernel(const MelinvArgs a)
{
    constexpr int NT = GROUPS * TF, ITEMS = (NBIN + GROUPS - 1) / GROUPS;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const Z = smem;                                  // [513][TF], float32 of the owners' Z
    float* const y = Z + NBIN * TF;                         // [80][TF]
    float* const r = y + NMEL * TF;                         // [80][TF]
    float* const cst = r + NMEL * TF;
    const int* const binf = reinterpret_cast<const int*>(cst + C_BINF);
    const float* const w0 = cst + C_W0;
    const float* const w1 = cst + C_W1;
    const int4* const filt = reinterpret_cast<const int4*>(cst + C_FILT);
    const float* const fw = cst + C_FW;

    const int tid = threadIdx.x, n = tid % TF, g = tid / TF;
    const int T = a.T, tiles_per = (T + TF - 1) / TF;
    const int b = blockIdx.x / tiles_per, t = (blockIdx.x % tiles_per) * TF + n;
    if (b >= a.B) return;
    const bool valid = t < T;                               // a frame past the end runs on y = 0 and is never stored

    for (int i = tid; i < CST_FLOATS; i += NT) cst[i] = a.tables[OFF_CST + i];
    for (int j = g; j < NMEL; j += GROUPS) y[j * TF + n] = valid ? exp10f(a.in[((long long)b * NMEL + j) * T + t]) : 0.f;
    __syncthreads();

    const float* const pinv = a.tables + OFF_PINV;
#pragma unroll 1
    for (int bin = g; bin < NBIN; bin += GROUPS) {
        float v = 0.f;
        for (int j = 0; j < NMEL; ++j) v = fmaf(pinv[bin * NMEL + j], y[j * TF + n], v);
        Z[bin * TF + n] = fmaxf(v, 0.f);
    }
    double m[ITEMS], z[ITEMS];                              // the thread's own bins (it wrote them itself: no barrier)
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const int bin = i * GROUPS + g;
        m[i] = z[i] = bin < NBIN ? (double)Z[bin * TF + n] : 0.0;
    }

    const double s = (double)a.tables[OFF_STEP];
#pragma unroll 1
    for (int k = 0; k < a.n_iter; ++k) {
        __syncthreads();                                    // Z_k is complete, r of the step before is read
#pragma unroll 1
        for (int rd = 0; rd < ROUNDS; ++rd) {
            const int j = rd * GROUPS + ((rd & 1) ? GROUPS - 1 - g : g);
            const int4 f = filt[j];                         // first bin, count, offset of the weights
            const float* const zp = Z + f.x * TF + n;
            const float* const wp = fw + f.z;
            float acc = 0.f;
            for (int c0 = 0; c0 < f.y; c0 += CHUNK) {       // loads of a chunk go out together; the chain keeps its order
                float wv[CHUNK], zv[CHUNK];
#pragma unroll
                for (int c = 0; c < CHUNK; ++c) {
                    const int cc = c0 + c < f.y ? c0 + c : f.y - 1;
                    wv[c] = wp[cc]; zv[c] = zp[cc * TF];
                }
#pragma unroll
                for (int c = 0; c < CHUNK; ++c) acc = c0 + c < f.y ? fmaf(wv[c], zv[c], acc) : acc;
            }
            r[j * TF + n] = acc - y[j * TF + n];
        }
        __syncthreads();
        const double beta = (double)a.tables[OFF_BETA + k];
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const int bin = i * GROUPS + g;
            if (i == ITEMS - 1 && bin >= NBIN) continue;    // (only the last item can lie past bin 512)
            const int f = binf[bin];
            const bool in_filter = f >= 0;                  // selects, not branches: the 33 items' loads overlap
            const int fi = in_filter ? f : 0;
            const float gr = fmaf(w1[bin], r[(fi + 1) * TF + n], w0[bin] * r[fi * TF + n]);
            const double mn = in_filter ? fmax(fma(-s, (double)gr, z[i]), 0.0) : m[i];
            z[i] = in_filter ? fma(beta, mn - m[i], mn) : z[i];
            m[i] = mn;
            Z[bin * TF + n] = (float)z[i];
        }
    }

    if (!valid) return;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const int bin = i * GROUPS + g;
        if (bin < NBIN) a.out[((long long)b * NBIN + bin) * T + t] = (float)m[i];
    }
}

bool shape_ok(int B, int T)                                 // the decoder's limits, from one frame on
{
    return B >= 1 && T >= 1 && T <= MCVC_GL_MAX_FRAMES && (long long)B * T <= (1LL << 22) && B <= 65535;
}

hipError_t launch(const MelinvArgs& a, hipStream_t s)
{
    static std::once_flag once;
    static hipError_t attr = hipSuccess;
    std::call_once(once, [] {
        attr = hipFuncSetAttribute(reinterpret_cast<const void*>(melinv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_FLOATS * 4);
    });
    if (attr != hipSuccess) return attr;
    const unsigned n_tiles = (unsigned)(a.B * cdiv_i(a.T, TF));
    hipLaunchKernelGGL(melinv_kernel, dim3(n_tiles), dim3(GROUPS * TF), LDS_FLOATS * 4, s, a);
    return hipGetLastError();
}

}  // namespace

long long mcvc_melinv_tables_floats_of() { return TABLE_FLOATS; }

int mcvc_melinv_tables_fill(const float* basis, const float* pinv, double lambda, float* out)
{
    if (!(lambda > 0.0) || !std::isfinite(lambda)) return MCVC_ERR_INVALID;
    for (int i = 0; i < NMEL * NBIN; ++i)
        if (!std::isfinite(basis[i])) return MCVC_ERR_INVALID;
    // every check runs before the first write: a refused call leaves host_out alone
    int first[NBIN], fbin[NMEL], fcnt[NMEL];
    float w[NBIN][2];
    for (int b = 0; b < NBIN; ++b) {
        int lo = -1, nz = 0;
        for (int j = 0; j < NMEL; ++j)
            if (basis[j * NBIN + b] != 0.f) {
                if (nz == 0) lo = j;
                else if (nz >= 2 || j != lo + 1) return MCVC_ERR_INVALID;      // a third non-zero, or two that are not neighbours
                ++nz;
            }
        first[b] = lo;
        w[b][0] = w[b][1] = 0.f;
        if (nz == 2) { w[b][0] = basis[lo * NBIN + b]; w[b][1] = basis[(lo + 1) * NBIN + b]; }
        else if (nz == 1 && lo == 0) w[b][0] = basis[b];
        else if (nz == 1) { first[b] = lo - 1; w[b][1] = basis[lo * NBIN + b]; }      // so that first + 1 is always a filter
    }
    for (int j = 0; j < NMEL; ++j) {
        int lo = 0, hi = -1;
        for (int b = 0; b < NBIN; ++b)
            if (basis[j * NBIN + b] != 0.f) { if (hi < 0) lo = b; hi = b; }
        fbin[j] = lo; fcnt[j] = hi < 0 ? 0 : hi - lo + 1;
        for (int b = lo; b <= hi; ++b)
            if (basis[j * NBIN + b] == 0.f) return MCVC_ERR_INVALID;           // a filter with a hole
    }
    for (long long i = 0; i < TABLE_FLOATS; ++i) out[i] = 0.f;
    for (int i = 0; i < NBIN * NMEL; ++i) out[OFF_PINV + i] = pinv[i];
    out[OFF_STEP] = (float)(1.0 / lambda);
    double t = 1.0;
    for (int k = 0; k < MCVC_MELINV_MAX_ITER; ++k) {
        const double tn = (1.0 + std::sqrt(1.0 + 4.0 * t * t)) / 2.0;
        out[OFF_BETA + k] = (float)((t - 1.0) / tn);
        t = tn;
    }
    float* const cst = out + OFF_CST;
    int* const binf = reinterpret_cast<int*>(cst + C_BINF);
    int* const filt = reinterpret_cast<int*>(cst + C_FILT);
    for (int b = 0; b < NBIN; ++b) { binf[b] = first[b]; cst[C_W0 + b] = w[b][0]; cst[C_W1 + b] = w[b][1]; }
    for (int b = NBIN; b < NBIN_LD; ++b) binf[b] = -1;
    int off = 0;
    for (int j = 0; j < NMEL; ++j) {
        filt[4 * j] = fbin[j]; filt[4 * j + 1] = fcnt[j]; filt[4 * j + 2] = off; filt[4 * j + 3] = 0;
        for (int c = 0; c < fcnt[j]; ++c) cst[C_FW + off + c] = basis[j * NBIN + fbin[j] + c];
        off += fcnt[j];                                     // at most 2 x 513: every bin counts in at most two filters
    }
    return MCVC_OK;
}

int mcvc_melinv_solve_launch(const float* logmel, const float* tables, float* mag_out, int B, int T, int n_iter, hipStream_t s)
{
    if (!logmel || !tables || !mag_out || !shape_ok(B, T) || n_iter < 0 || n_iter > MCVC_MELINV_MAX_ITER) return MCVC_ERR_INVALID;
    if (((uintptr_t)logmel & 3) || ((uintptr_t)tables & 15) || ((uintptr_t)mag_out & 3)) return MCVC_ERR_INVALID;
    MelinvArgs a{};
    a.in = logmel; a.tables = tables; a.out = mag_out; a.B = B; a.T = T; a.n_iter = n_iter;
    const double F = (double)B * T;
    TraceScope ts(K_ELEMENTWISE, s, F * (2.0 * NBIN * NMEL + n_iter * (4.0 * 2 * NBIN + 6.0 * NBIN)), 4.0 * F * (NMEL + NBIN));
    return (int)launch(a, s);
}
