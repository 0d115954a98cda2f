// Objective evaluation: mel-cepstral distortion after dynamic-time-warping alignment (definitions: mask_cyclegan_vc/metrics.py).
//
//   cep_project_kernel    c[k][n] = sum_m B[k][m] * (ln 10 * mel[m][n]),  k = 1 .. n_cep, over a whole [80][N] bank in one launch.
//   dtw_kernel<KC>        one WAVEFRONT per pair (one 64-thread workgroup each, any mix of lengths in one launch).  The Tx rows are cut into
//                         strips of 64; lane l owns row 64 strip + l and sweeps the columns skewed: in step s it is at column s - l.  So
//                           left  (i, j-1)   = the lane's own value of the step before,
//                           up    (i-1, j)   = lane l-1's value of the step before      (one lane move),
//                           diag  (i-1, j-1) = the `up` this lane received one step earlier,
//                         and lane 0 takes up / diag from the boundary row the strip before left in LDS (lane 63 writes column s - 63 while
//                         lane 0 reads column s + 1: the buffer is reused in place).  d(i, j) does not depend on the recurrence: x's rows sit in
//                         registers, y's column values of step s + 2 are in flight and d of step s + 1 is computed while the chain of step s
//                         (two compares, two selects, one add, the lane moves) runs.  No wave waits for another one: a pair is one wave from
//                         its first to its last strip, and __syncthreads() of a one-wave workgroup only orders the LDS hand-off.
//                         Absent predecessors carry +inf (a virtual cell (-1, -1) = 0 starts the recurrence), so the tie rule -- diag, up, left,
//                         replaced on strict < -- needs no special cases.  len is carried with acc; with want_path one direction byte per cell
//                         goes to the workspace in sweep order (strip, step, lane): 64 consecutive bytes per step.
//   dtw_backtrack_kernel  the second launch (the kernel boundary orders it after the direction stores): one thread per pair walks the stored
//                         directions from (Tx-1, Ty-1) and writes row length-1-n of the pair's path.  At most Tx + Ty - 1 steps whatever the bytes hold.
// Every trip count is a function of the lengths alone.
#include <cmath>
#include <cstdint>
#include <limits>

#include "dtw.h"
#include "mcvc_common.h"
#include "trace.h"

namespace {

constexpr int MAXF = MCVC_DTW_MAX_FRAMES, NMEL = MCVC_CEP_NMEL, COLS = MCVC_DTW_TABLE_COLS;
constexpr int CEP_THREADS = 256;
constexpr double kPi = 3.14159265358979323846;

struct DtwArgs {
    const float* x; const float* y;
    const long long* table;
    float* cost; int* length; int* path;
    unsigned char* dirs;             // null: no path wanted
    long long nx, ny, ws_bytes, path_rows;
    float scale;
    int K, n_pairs;
};

struct Pair { long long xo, yo, dir_off, path_off; int Tx, Ty; bool ok; };

__device__ __host__ inline long long dir_bytes_of(long long Tx, long long Ty) { return ((Tx + 63) / 64) * (Ty + 63) * 64; }

// What the plan guarantees, checked again: a row that does not describe these banks reads and writes nothing.
__device__ inline Pair load_pair(const DtwArgs& a, int p, bool want_path)
{
    const long long* r = a.table + (long long)COLS * p;
    Pair q;
    const long long Tx = r[1], Ty = r[3];
    q.xo = r[0]; q.yo = r[2]; q.dir_off = r[4]; q.path_off = r[5];
    q.ok = q.xo >= 0 && Tx >= 1 && Tx <= MAXF && q.xo + Tx <= a.nx && q.yo >= 0 && Ty >= 1 && Ty <= MAXF && q.yo + Ty <= a.ny;
    if (q.ok && a.dirs) q.ok = q.dir_off >= 0 && q.dir_off + dir_bytes_of(Tx, Ty) <= a.ws_bytes;
    if (q.ok && want_path) q.ok = a.dirs && q.path_off >= 0 && q.path_off + Tx + Ty - 1 <= a.path_rows;
    q.Tx = q.ok ? (int)Tx : 0; q.Ty = q.ok ? (int)Ty : 0;
    return q;
}

// KC: K in (8 KC - 8, 8 KC].  Only the last eight feature rows are selected against K at run time (a select per row costs a mask).
template <int KC>
__global__ __launch_bounds__(64) void dtw_kernel(DtwArgs a)
{
    constexpr int KT = 8 * KC, KF = KT - 8;
    __shared__ float bnd_acc[MAXF];
    __shared__ int bnd_len[MAXF];
    const int p = blockIdx.x, lane = threadIdx.x;
    const Pair q = load_pair(a, p, false);
    if (!q.ok) {                                               // (uniform: the whole wave leaves)
        if (lane == 0) { a.cost[p] = std::numeric_limits<float>::quiet_NaN(); a.length[p] = 0; }
        return;
    }
    const int Tx = q.Tx, Ty = q.Ty, K = a.K;
    const float INF = std::numeric_limits<float>::infinity();
    const char* xb = reinterpret_cast<const char*>(a.x + q.xo);
    const char* yb = reinterpret_cast<const char*>(a.y + q.yo);
    const unsigned nx4 = (unsigned)(a.nx * 4), ny4 = (unsigned)(a.ny * 4);
    const int nstrips = (Tx + 63) >> 6, W = Ty + 63;
    const float scale = a.scale;
    unsigned char* dirs = a.dirs ? a.dirs + q.dir_off : nullptr;
    float cur_acc = INF;
    int cur_len = 0;

    for (int strip = 0; strip < nstrips; ++strip) {
        const int i = strip * 64 + lane;
        const bool row_ok = i < Tx;
        const int ic = row_ok ? i : Tx - 1;
        const int rows = min(64, Tx - strip * 64);
        const int nsteps = Ty + rows - 1;
        float xr[KT], yv[KT];
        {
            unsigned off = (unsigned)ic * 4u;
#pragma unroll
            for (int k = 0; k < KT; ++k) {                     // rows beyond K: the last row again, never used
                xr[k] = *reinterpret_cast<const float*>(xb + off);
                off += (k + 1 < KF || k + 1 < K) ? nx4 : 0u;
            }
        }
        auto load_y = [&](int s) {                             // lanes of a step touch consecutive addresses of every row of y
            const int jc = min(max(s - lane, 0), Ty - 1);
            unsigned off = (unsigned)jc * 4u;                  // one uniform base + a 32-bit byte offset per lane (a bank is under 4 GB)
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                yv[k] = *reinterpret_cast<const float*>(yb + off);
                off += (k + 1 < KF || k + 1 < K) ? ny4 : 0u;
            }
        };
        auto dist = [&]() {                                    // from differences, summed in the order of k
            float sum = 0.0f;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                float d = xr[k] - yv[k];
                if (!(k < KF || k < K)) d = 0.0f;              // (selected where it is used: the loads stay in flight for a whole step)
                sum = fmaf(d, d, sum);
            }
            return scale * sqrtf(sum);
        };
        load_y(0);
        float d_cur = dist();
        load_y(1);
        cur_acc = INF; cur_len = 0;
        float dg_acc = (strip == 0 && lane == 0) ? 0.0f : INF;  // the virtual cell (-1, -1): acc 0, len 0
        int dg_len = 0;
        float b_acc = INF;
        int b_len = 0;
        if (strip > 0) { b_acc = bnd_acc[0]; b_len = bnd_len[0]; }
        for (int s = 0; s < nsteps; ++s) {
            const float d_next = dist();                       // step s + 1
            load_y(s + 2);
            float nb_acc = INF;
            int nb_len = 0;
            if (strip > 0) { const int jn = min(s + 1, Ty - 1); nb_acc = bnd_acc[jn]; nb_len = bnd_len[jn]; }
            // ---- the dependent chain of step s
            float up_acc = __shfl_up(cur_acc, 1);
            int up_len = __shfl_up(cur_len, 1);
            if (lane == 0) { up_acc = b_acc; up_len = b_len; }
            const int j = s - lane;
            const bool active = row_ok && j >= 0 && j < Ty;
            float best = dg_acc;
            int bl = dg_len, dir = 0;
            if (up_acc < best) { best = up_acc; bl = up_len; dir = 1; }
            if (cur_acc < best) { best = cur_acc; bl = cur_len; dir = 2; }
            if (active) {
                cur_acc = d_cur + best;
                cur_len = bl + 1;
                if (dirs) dirs[((long long)strip * W + s) * 64 + lane] = (unsigned char)dir;
                if (lane == 63) { bnd_acc[j] = cur_acc; bnd_len[j] = cur_len; }
            }
            dg_acc = up_acc; dg_len = up_len;
            b_acc = nb_acc; b_len = nb_len;
            d_cur = d_next;
        }
        __syncthreads();                                       // one wave: orders lane 63's boundary row before the next strip's reads
    }
    if (lane == ((Tx - 1) & 63)) { a.cost[p] = cur_acc; a.length[p] = cur_len; }
}

__global__ __launch_bounds__(64) void dtw_backtrack_kernel(DtwArgs a)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= a.n_pairs) return;
    const Pair q = load_pair(a, p, true);
    if (!q.ok) return;
    const int Tx = q.Tx, Ty = q.Ty, W = Ty + 63, cap = Tx + Ty - 1;
    const unsigned char* dirs = a.dirs + q.dir_off;
    int* path = a.path + 2 * q.path_off;
    const int len = a.length[p];
    int i = Tx - 1, j = Ty - 1;
    for (int n = 0; n < cap; ++n) {                            // every step lowers i or j: at most Tx + Ty - 1 rows, whatever the bytes hold
        const int k = len - 1 - n;
        if (k >= 0 && k < cap) { path[2 * k] = i; path[2 * k + 1] = j; }
        if (i == 0 && j == 0) break;
        int dir = dirs[((long long)(i >> 6) * W + j + (i & 63)) * 64 + (i & 63)];
        if (i == 0) dir = 2; else if (j == 0) dir = 1;
        if (dir == 0) { --i; --j; } else if (dir == 1) --i; else --j;
    }
}

__global__ __launch_bounds__(CEP_THREADS) void cep_project_kernel(const float* __restrict__ mel, long long N, const float* __restrict__ basis, int n_cep,
                                                                   float* __restrict__ out)
{
    __shared__ float B[MCVC_CEP_MAX * NMEL];
    for (int i = threadIdx.x; i < n_cep * NMEL; i += CEP_THREADS) B[i] = basis[i];
    __syncthreads();
    const long long n = (long long)blockIdx.x * CEP_THREADS + threadIdx.x;
    if (n >= N) return;
    const float LN10 = 2.302585092994046f;
    float v[NMEL];
#pragma unroll
    for (int m = 0; m < NMEL; ++m) v[m] = LN10 * mel[(long long)m * N + n];
    for (int k = 0; k < n_cep; ++k) {
        float acc = 0.0f;
#pragma unroll
        for (int m = 0; m < NMEL; ++m) acc = fmaf(B[k * NMEL + m], v[m], acc);
        out[(long long)k * N + n] = acc;
    }
}

}  // namespace

int mcvc_cep_basis_fill(int n_cep, float* host)
{
    if (n_cep < 1 || n_cep > MCVC_CEP_MAX || !host) return MCVC_ERR_INVALID;
    const double c = std::sqrt(2.0 / NMEL);
    for (int k = 1; k <= n_cep; ++k)
        for (int m = 0; m < NMEL; ++m) {
            const int ph = (int)(((long long)(2 * m + 1) * k) % (4 * NMEL));      // cos(pi (2m + 1) k / 160), argument reduced exactly
            host[(k - 1) * NMEL + m] = (float)(c * std::cos(kPi * ph / (2.0 * NMEL)));
        }
    return MCVC_OK;
}

int mcvc_cep_project_launch(const float* mel, long long n_frames, const float* basis, int n_cep, float* out, hipStream_t s)
{
    if (!mel || !basis || !out || n_frames < 1 || n_frames > 0x7fffffffLL || n_cep < 1 || n_cep > MCVC_CEP_MAX) return MCVC_ERR_INVALID;
    if (((uintptr_t)mel & 3) || ((uintptr_t)out & 3) || ((uintptr_t)basis & 15)) return MCVC_ERR_INVALID;
    TraceScope ts(K_SGEMM, s, 2.0 * n_cep * NMEL * (double)n_frames, 4.0 * (NMEL + n_cep) * (double)n_frames);
    hipLaunchKernelGGL(cep_project_kernel, dim3((unsigned)cdiv_ll(n_frames, CEP_THREADS)), dim3(CEP_THREADS), 0, s, mel, n_frames, basis, n_cep, out);
    return (int)hipGetLastError();
}

int mcvc_dtw_plan_host(const int* x_offs, const int* y_offs, int n_pairs, int want_path, long long* table, long long* ws_bytes, long long* path_rows)
{
    if (!x_offs || !y_offs || n_pairs < 1 || !ws_bytes || !path_rows || x_offs[0] < 0 || y_offs[0] < 0) return MCVC_ERR_INVALID;
    long long ws = 0, rows = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const long long Tx = (long long)x_offs[p + 1] - x_offs[p], Ty = (long long)y_offs[p + 1] - y_offs[p];
        if (Tx < 1 || Tx > MAXF || Ty < 1 || Ty > MAXF) return MCVC_ERR_INVALID;      // (also: offsets that do not rise)
        if (table) {
            long long* r = table + (long long)COLS * p;
            r[0] = x_offs[p]; r[1] = Tx; r[2] = y_offs[p]; r[3] = Ty; r[4] = want_path ? ws : -1; r[5] = want_path ? rows : -1;
        }
        if (want_path) { ws += dir_bytes_of(Tx, Ty); rows += Tx + Ty - 1; }
    }
    *ws_bytes = ws; *path_rows = rows;
    return MCVC_OK;
}

int mcvc_dtw_run_launch(const float* x, long long x_frames, const float* y, long long y_frames, int K, float scale, const int* x_offs_host,
                        const int* y_offs_host, const long long* table, int n_pairs, float* cost, int* length, int* path, void* ws,
                        long long ws_bytes, hipStream_t s)
{
    if (!x || !y || !table || !cost || !length || K < 1 || K > MCVC_DTW_MAX_K || n_pairs < 1 || !(scale == scale)) return MCVC_ERR_INVALID;
    if (((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)cost & 3) || ((uintptr_t)length & 3) || ((uintptr_t)path & 3)) return MCVC_ERR_INVALID;
    if (((uintptr_t)table & 15) || ((uintptr_t)ws & 15)) return MCVC_ERR_INVALID;
    long long need = 0, rows = 0;
    const int rc = mcvc_dtw_plan_host(x_offs_host, y_offs_host, n_pairs, path != nullptr, nullptr, &need, &rows);
    if (rc != MCVC_OK) return rc;
    if (x_offs_host[n_pairs] > x_frames || y_offs_host[n_pairs] > y_frames) return MCVC_ERR_INVALID;
    if ((long long)K * x_frames > 0x3fffffffLL || (long long)K * y_frames > 0x3fffffffLL) return MCVC_ERR_INVALID;   // 32-bit byte offsets inside a bank
    if (need > 0 && (!ws || ws_bytes < need)) return MCVC_ERR_WORKSPACE;
    DtwArgs a{};
    a.x = x; a.y = y; a.table = table; a.cost = cost; a.length = length; a.path = path;
    a.dirs = path ? static_cast<unsigned char*>(ws) : nullptr;
    a.nx = x_frames; a.ny = y_frames; a.ws_bytes = path ? need : 0; a.path_rows = rows; a.scale = scale; a.K = K; a.n_pairs = n_pairs;
    double cells = 0.0;
    for (int p = 0; p < n_pairs; ++p)
        cells += (double)(x_offs_host[p + 1] - x_offs_host[p]) * (double)(y_offs_host[p + 1] - y_offs_host[p]);
    {
        TraceScope ts(K_ELEMENTWISE, s, cells * (3.0 * K + 6.0), 4.0 * K * (double)(x_frames + y_frames) + (path ? cells : 0.0));
        const dim3 grid((unsigned)n_pairs), block(64);
        switch ((K + 7) / 8) {
#define MCVC_DTW_CASE(KC) case KC: hipLaunchKernelGGL(dtw_kernel<KC>, grid, block, 0, s, a); break;
            MCVC_DTW_CASE(1) MCVC_DTW_CASE(2) MCVC_DTW_CASE(3) MCVC_DTW_CASE(4) MCVC_DTW_CASE(5)
            MCVC_DTW_CASE(6) MCVC_DTW_CASE(7) MCVC_DTW_CASE(8) MCVC_DTW_CASE(9) MCVC_DTW_CASE(10)
#undef MCVC_DTW_CASE
            default: return MCVC_ERR_INVALID;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    if (path) {
        TraceScope ts(K_ELEMENTWISE, s, 0.0, (double)rows * 9.0);
        hipLaunchKernelGGL(dtw_backtrack_kernel, dim3((unsigned)cdiv_i(n_pairs, 64)), dim3(64), 0, s, a);
        return (int)hipGetLastError();
    }
    return MCVC_OK;
}
