// Sample-rate conversion of a ragged bank of utterances: scipy.signal.resample_poly's default filter (Kaiser 5.0 windowed sinc of
// 20 max(up, down) + 1 taps, zero padding) in polyphase form (definition: include/mcvc.h; data_preprocessing/resample.py makes the taps;
// tests/resample_checker.py restates the transform in float64).
//
//   resample_kernel   one workgroup of 256 threads per ROW of mcvc_resample_plan's work list: up to 1024 consecutive output samples of one
//                     utterance.  With c = k down + half, q = c div up, r = c mod up:   y[k] = sum_{j < J} P[r][j] x[q - j].
//                     The plan computes (q0, r0) of the row's first output in 64 bits; output i of the row has t = r0 + i down < 2^20,
//                     q = q0 + t div up, r = t mod up: small integers from there on.
//                     The row's input span x[q0 - J + 1 .. q_last] is staged in LDS, zero outside [0, n_in) of ITS utterance (never the
//                     neighbour's samples, never the buffer's bounds), then every thread forms outputs tid, tid + 256, ... as J fused
//                     multiply-adds in the order j = 0 .. J - 1: one order per output whatever shares the row or the bank with it.
//   The polyphase table lives in LDS too, not behind L2: neighbouring lanes need DIFFERENT rows r (they differ by down mod up), so through
//   the vector cache every step of j would be a 64-way gather over a 26 .. 55 KB table that does not fit the 32 KB L1; in LDS a gather costs
//   only its bank conflicts.  Copying it in costs up (J | 1) floats per row, coalesced and from L2: 6.5 floats per output at 48 -> 22.05 kHz
//   with full rows, which is why a row holds 1024 outputs and not 256.  Table (<= 55 KB) + span (<= 64 KB) fit the 160 KB of a CU; the
//   launch asks for what its rows need (28 KB at 48 -> 22.05 kHz: five workgroups per CU).
//   Bank pattern (a 32-bit ds_read banks at (address / 4) mod 32 within each half of 32 lanes).  Lane i reads table[r_i S + j] with
//   r_i = (r0 + i down) mod up.  With the natural pitch S = J an even J loses banks: counted over every half-wave of a full row
//   (tools/resample_bench.py --banks prints the table), 48 -> 22.05 kHz (147/320, S = 44) is 6-way, 96 -> 22.05 kHz (S = 88) 9-way,
//   22.05 -> 8 kHz (160/441, S = 56) 8-way, 22.05 -> 16 kHz (S = 28) 4-way.  An ODD pitch S = J | 1 makes r -> r S mod 32 a bijection of
//   r mod 32, so lanes collide only where their r agree mod 32: every pair between 22050 Hz and the ten supported rates is then
//   conflict-free or 2-way, except 8 -> 22.05 kHz (441/160), which is 3-way; 1/2, 2/1, 1/4, 4/1 read one to four rows (broadcasts).
//   The x reads advance by down / up samples per lane: conflict-free when upsampling (same or neighbouring words), 2-way when
//   decimating by up to 4.4 : 1 (4-way at exactly 4 : 1), which the 20 to 88 multiply-adds per output leave under the stream from HBM.
// No atomics, no workspace, no device allocation.
#include <climits>
#include <cstdint>

#include "mcvc_common.h"
#include "resample.h"
#include "trace.h"

namespace {

constexpr int MAXF = MCVC_RESAMPLE_MAX_FACTOR, TILE = MCVC_RESAMPLE_TILE, COLS = MCVC_RESAMPLE_TILE_COLS, SPAN_MAX = MCVC_RESAMPLE_SPAN_MAX;
constexpr int THREADS = 256;
constexpr int TABLE_MAX = 22 * MAXF;                           // up (J | 1) <= 20 m + 2 up
static_assert((long long)(MAXF - 1) + (long long)(TILE - 1) * MAXF < (1LL << 30), "a row's phase counter stays a small int");
static_assert((TABLE_MAX + SPAN_MAX) * 4 <= 160 * 1024 && TABLE_MAX % 4 == 0, "table and span share one CU's LDS");

struct Ratio {
    int up, down, half, J, S;
    long long table_floats;
    bool ok;
};

inline int gcd_i(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// any 1 <= up, down <= MAXF: what sizing and packing need; the plan and the launch also want up != down and gcd 1
inline Ratio ratio_of(int up, int down)
{
    Ratio r{up, down, 0, 0, 0, 0, false};
    if (up < 1 || down < 1 || up > MAXF || down > MAXF) return r;
    const int m = up > down ? up : down;
    r.half = 10 * m;
    r.J = (2 * r.half + 1 + up - 1) / up;
    r.S = r.J | 1;
    r.table_floats = ((long long)up * r.S + 3) / 4 * 4;
    r.ok = true;
    return r;
}

inline bool coprime_pair(const Ratio& r) { return r.ok && r.up != r.down && gcd_i(r.up, r.down) == 1; }

// staged input samples of a row of n outputs that starts at phase r0
inline long long span_of(const Ratio& r, int r0, int n) { return ((long long)r0 + (long long)(n - 1) * r.down) / r.up + r.J; }

// most outputs of a row whatever its phase: span_of(up - 1, n) <= SPAN_MAX
inline int row_outputs(const Ratio& r)
{
    const long long n = ((long long)(SPAN_MAX - r.J) * r.up - (r.up - 1)) / r.down + 1;
    return n > TILE ? TILE : (n < 1 ? 1 : (int)n);
}

struct RsArgs {
    const float* x;
    const int* tiles;          // [n_tiles][8]: in_off, n_in, out0, n, q0, r0, 0, 0
    const float* table;        // [up][S], padded to 4 floats
    float* y;
    long long n_in_total, n_out_total;
    int up, down, J, S, table_floats;
};

__global__ __launch_bounds__(THREADS) void resample_kernel(const RsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const int4 ta = reinterpret_cast<const int4*>(a.tiles)[2 * blockIdx.x], tb = reinterpret_cast<const int4*>(a.tiles)[2 * blockIdx.x + 1];
    const int in_off = ta.x, n_in = ta.y, out0 = ta.z, n = ta.w, q0 = tb.x, r0 = tb.y;
    const int up = a.up, down = a.down, J = a.J, S = a.S;
    // what the launch checked on the host, once more (uniform: the whole workgroup leaves before its first barrier)
    if (in_off < 0 || n_in < 1 || (long long)in_off + n_in > a.n_in_total || out0 < 0 || n < 1 || n > TILE || (long long)out0 + n > a.n_out_total ||
        q0 < 0 || r0 < 0 || r0 >= up)
        return;
    const int span = (r0 + (n - 1) * down) / up + J;
    if (span > SPAN_MAX) return;

    float* const tab = smem;
    float* const xs = smem + a.table_floats;
    const float4* const tsrc = reinterpret_cast<const float4*>(a.table);
    for (int i = tid; i < a.table_floats / 4; i += THREADS) reinterpret_cast<float4*>(tab)[i] = tsrc[i];
    // ---- the row's samples x[lo .. lo + span): zero outside [0, n_in) of this utterance ----
    const float* const src = a.x + in_off;
    const long long lo = (long long)q0 - J + 1;
    for (int p = tid; p < span; p += THREADS) {
        const long long g = lo + p;
        xs[p] = (g >= 0 && g < n_in) ? src[g] : 0.f;
    }
    __syncthreads();

    float* const dst = a.y + out0;
    for (int i = tid; i < n; i += THREADS) {
        const int t = r0 + i * down, dq = t / up, r = t - dq * up;
        const float* const P = tab + r * S;
        const float* const xp = xs + dq + J - 1;                // x[q]: q - lo = dq + J - 1 <= span - 1
        float acc = 0.f;
        for (int j = 0; j < J; ++j) acc = fmaf(P[j], xp[-j], acc);
        dst[i] = acc;
    }
}

}  // namespace

long long mcvc_resample_out_samples_of(long long n_in, int up, int down)
{
    const Ratio r = ratio_of(up, down);
    if (!r.ok || n_in < 1 || n_in > (LLONG_MAX - down) / up) return 0;
    return (n_in * up + down - 1) / down;
}

long long mcvc_resample_table_floats_of(int up, int down) { return ratio_of(up, down).table_floats; }

int mcvc_resample_pack_host(const float* h, int n_taps, int up, int down, float* table)
{
    const Ratio r = ratio_of(up, down);
    if (!h || !table || !r.ok || n_taps != 2 * r.half + 1) return MCVC_ERR_INVALID;
    for (long long i = 0; i < r.table_floats; ++i) table[i] = 0.f;
    for (int n = 0; n < n_taps; ++n) table[(long long)(n % up) * r.S + n / up] = h[n];
    return MCVC_OK;
}

int mcvc_resample_plan_host(const int* in_offs, int n_utts, int up, int down, int* out_offs, int* tiles, int max_tiles, int* n_tiles_out)
{
    const Ratio r = ratio_of(up, down);
    if (!in_offs || !out_offs || !n_tiles_out || n_utts < 1 || !coprime_pair(r) || in_offs[0] < 0 || (tiles && max_tiles < 0)) return MCVC_ERR_INVALID;
    const int rows = row_outputs(r);
    long long total = 0, count = 0;
    for (int u = 0; u < n_utts; ++u) {
        const long long n_in = (long long)in_offs[u + 1] - in_offs[u];
        if (n_in < 1) return MCVC_ERR_INVALID;
        const long long n_out = (n_in * up + down - 1) / down;
        if (total + n_out >= (1LL << 31)) return MCVC_ERR_INVALID;
        total += n_out;
        count += (n_out + rows - 1) / rows;
    }
    if (count > INT_MAX) return MCVC_ERR_INVALID;
    // (q of a row's first output stays under n_in + (half + down) / up + 1 <= 2^31 + 12801: refuse the sliver that would not fit an int)
    long long out = 0, row = 0;
    for (int u = 0; u < n_utts; ++u) {
        const long long n_in = (long long)in_offs[u + 1] - in_offs[u];
        const long long n_out = (n_in * up + down - 1) / down;
        out_offs[u] = (int)out;
        for (long long k = 0; k < n_out; k += rows, ++row) {
            const long long c = k * down + r.half, q = c / up;
            if (q > INT_MAX) return MCVC_ERR_INVALID;
            if (tiles && row < max_tiles) {
                int* const t = tiles + COLS * row;
                t[0] = in_offs[u]; t[1] = (int)n_in; t[2] = (int)(out + k); t[3] = (int)(n_out - k < rows ? n_out - k : rows);
                t[4] = (int)q; t[5] = (int)(c % up); t[6] = 0; t[7] = 0;
            }
        }
        out += n_out;
    }
    out_offs[n_utts] = (int)out;
    *n_tiles_out = (int)count;
    return tiles && max_tiles < count ? MCVC_ERR_WORKSPACE : MCVC_OK;
}

int mcvc_resample_run_launch(const float* x, long long n_in_total, const int* tiles, int n_tiles, const float* table, int up, int down, float* y,
                             long long n_out_total, hipStream_t s)
{
    const Ratio r = ratio_of(up, down);
    if (!x || !tiles || !table || !y || !coprime_pair(r) || n_tiles < 1 || n_in_total < 1 || n_out_total < 1 || n_in_total > INT_MAX || n_out_total > INT_MAX)
        return MCVC_ERR_INVALID;
    if (((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)table & 15) || ((uintptr_t)tiles & 15)) return MCVC_ERR_INVALID;
    // the work list is read here AND by the kernel: pinned host memory, through its device mapping
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, tiles) != hipSuccess) { (void)hipGetLastError(); return MCVC_ERR_INVALID; }
    if (at.type != hipMemoryTypeHost || !at.hostPointer || !at.devicePointer) return MCVC_ERR_INVALID;
    const int* const rows = static_cast<const int*>(at.hostPointer);
    long long span_max = 0;
    for (int i = 0; i < n_tiles; ++i) {
        const int* const t = rows + COLS * (long long)i;
        const long long in_off = t[0], n_in = t[1], out0 = t[2], n = t[3], q0 = t[4], r0 = t[5];
        if (in_off < 0 || n_in < 1 || in_off + n_in > n_in_total || out0 < 0 || n < 1 || n > TILE || out0 + n > n_out_total || q0 < 0 || r0 < 0 || r0 >= up)
            return MCVC_ERR_INVALID;
        const long long span = span_of(r, (int)r0, (int)n);
        if (span > SPAN_MAX) return MCVC_ERR_INVALID;
        if (span > span_max) span_max = span;
    }
    static hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(resample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (TABLE_MAX + SPAN_MAX) * 4);
    if (attr != hipSuccess) return (int)attr;
    const RsArgs a{x, static_cast<const int*>(at.devicePointer), table, y, n_in_total, n_out_total, up, down, r.J, r.S, (int)r.table_floats};
    const size_t lds = (size_t)(r.table_floats + span_max) * 4;
    TraceScope ts(K_ELEMENTWISE, s, 2.0 * r.J * (double)n_out_total, 4.0 * ((double)n_in_total + (double)n_out_total));
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)n_tiles), dim3(THREADS), lds, s, a);
    return (int)hipGetLastError();
}
