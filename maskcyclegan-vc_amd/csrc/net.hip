// Network-level schedule of the MaskCycleGAN-VC Generator / Discriminator on the gfx950 kernels and
// the exported C ABI (include/mcvc.h).  The library owns the layer schedule so that one host call
// launches a whole forward or backward pass back-to-back on the caller's HIP stream (graph-capturable:
// no allocation, no synchronisation, no host-side state).
//
// Layer walk follows mask_cyclegan_vc/model.py:239-280 (Generator.forward) and :340-349
// (Discriminator.forward); parameter indices follow named_parameters() order.
//
// Internal layouts (all fp32):
//   2-D activations  NCHW  [B][C][H][W]
//   1-D trunk        [C][B][T4]  -- channel-major with the batch inside, so every Conv1d is a
//                    single-image KHx1 convolution over an image of B rows; the reference's
//                    view(B, 5120, 1, -1) (model.py:249-251, channel = c*20 + h) and view(B,256,20,-1)
//                    (:270-271) become pure stride changes folded into the producing kernels.
//   value|gate pairs are one convolution with concatenated output channels [value C | gate C].
#include "mcvc_common.h"
#include "twin.h"
#include "pack.h"
#include "packforms.h"
#include "misc.h"
#include "trunk.h"
#include "wino.h"
#include "wino4.h"
#include "sgemm.h"
#include "sampler.h"
#include "audio.h"
#include "vocoder.h"
#include "griffinlim.h"
#include "melinv.h"
#include "dtw.h"
#include "ms.h"
#include "f0.h"
#include "resample.h"
#include "vad.h"
#include "../../include/mcvc.h"
#include <string.h>
#include <algorithm>
#include <array>
#include <tuple>
#include <map>
#include <mutex>
#include <vector>

static int g_deterministic = [] { const char* e = getenv("MCVC_DETERMINISTIC"); return (e && atoi(e) != 0) ? 1 : 0; }();
int mcvc_deterministic() { return g_deterministic; }

namespace {

constexpr float kInEps = 1e-5f;

// A tensor as the kernels address it: N samples of C channels of H x W, sample / channel / row strides in floats (columns contiguous).
// The layouts the passes use are the named constructors below, each written once; what a wrapper needs beside the pointer -- the
// sample count, the image size, the dense size that spaces K-split slabs -- it reads off the tensor.
enum Layout { L_STRIDED, L_PHASE_SPLIT, L_PADDED_DY };
template <class T> struct TensorT {
    T* p; int N, C, H, W; long long sb, sc; int sh; Layout lay;
    operator TensorT<const T>() const { return {p, N, C, H, W, sb, sc, sh, lay}; }
    int P() const { return H * W; }
    long long dense() const { return (long long)N * C * H * W; }                 // slab stride of a K split that writes this tensor
    TensorT at(T* q) const { TensorT t = *this; t.p = q; return t; }             // the same shape elsewhere
    TensorT channels(int c0, int n) const { TensorT t = *this; t.p = p + c0 * sc; t.C = n; return t; }
    TensorT samples(int b0, int n) const { TensorT t = *this; t.p = p + b0 * sb; t.N = n; return t; }
    // trunk layout only: the B rows of a channel as ONE image of B rows (every Conv1d is a single-image convolution) ...
    TensorT image() const { return {p, 1, C, N, W, 0, sc, sh, lay}; }
    // ... and 20 consecutive channels as the rows of one (channel = c * 20 + h: the reference's view(B, 5120, 1, -1))
    TensorT rows20() const { return {p, N, C / 20, 20, W, sb, 20 * sc, (int)sc, lay}; }
    // dense planes only: every row a channel of its own (H x W -> H channels of 1 x W)
    TensorT rows_as_channels() const { return {p, N, C * H, 1, W, sb, (long long)sh, sh, lay}; }
};
using Tensor = TensorT<float>;
using CTensor = TensorT<const float>;
// dense, batch-major [N][C][H][W]
template <class T> static TensorT<T> nchw(T* p, int N, int C, int H, int W) { return {p, N, C, H, W, (long long)C * H * W, (long long)H * W, W, L_STRIDED}; }
// a dense buffer of n floats as one row (the in-place slab sums of the op-level entries)
template <class T> static TensorT<T> flat(T* p, long long n) { return nchw(p, 1, 1, 1, (int)n); }
// 1-D trunk layout [C][rows][W4], per sample: B samples W4 apart; channel pitch = rows x W4 of the buffer (the stash's rows: stash_B)
template <class T> static TensorT<T> trunk_rows(T* p, int B, int C, int W4, long long pitch) { return {p, B, C, 1, W4, (long long)W4, pitch, W4, L_STRIDED}; }
// input of a 3x3 stride-2 layer in the phase-split padded layout (sgemm.h): four padded phase planes per channel; H x W = the image
template <class T> static TensorT<T> phase_split(T* p, int N, int C, int H, int W)
{ const long long pl = mcvc_xs_plane(H, W); return {p, N, C, H, W, C * 4 * pl, 4 * pl, W, L_PHASE_SPLIT}; }
// dY of such a layer in the padded layout its implicit data gradient gathers from: planes of (OH + 1) rows of OW + 4 floats
template <class T> static TensorT<T> padded_dy(T* p, int N, int C, int OH, int OW)
{ const long long pl = mcvc_dyp_plane(OH, OW); return {p, N, C, OH, OW, C * pl, pl, mcvc_dyp_pitch(OW), L_PADDED_DY}; }
// the direct kernels' operands
static ConvIO conv_io(CTensor x, Tensor y)
{
    ConvIO io{};
    io.x = x.p; io.x_sb = x.sb; io.x_sc = x.sc; io.x_sh = x.sh;
    io.y = y.p; io.y_sb = y.sb; io.y_sc = y.sc; io.y_sh = y.sh; io.y_sw = 1;
    return io;
}

constexpr int kMaxLayers = 20;
struct PackFresh { unsigned layer[kMaxLayers]; PackFresh() { for (unsigned& m : layer) m = kAllForms; } };

struct Exec {
    hipStream_t s;
    bool dry;
    int err;
    bool fine_ms = false;          // generator backward: four milestones (flags & MCVC_BWD_FINE_MILESTONES), see gen_backward_impl
    float* slabs;
    long long slab_cap;
    long long slab_need;
    int max_split;                 // 0 = planner default (<= 64)
    // weight gradients are off the critical path of a backward pass: with an auxiliary stream they run beside the
    // data-gradient chain.  `readers` remembers, per dY buffer, the event after which its last aux-stream reader is done.
    hipStream_t s2;
    float* wslabs;
    long long wslab_cap;
    long long wslab_need;
    float* wv; float* wm;          // Winograd scratch: transformed input V[36][K][tiles], products M[36][M][tiles]
    long long wino_cap;            // floats available in each
    float* wv2; float* wm2; float* wu;   // the weight-gradient's own set (it runs on the auxiliary stream beside the dgrad): Vt, dMt, dU
    long long wu_cap;
    float* sg; long long sg_cap, sg_need;    // staging region of the staged-GEMM convolutions (sgemm.h): forward / data gradient (main stream)
    float* sgw; long long sgw_cap, sgw_need; // ... and the weight gradients' own (they may run on the auxiliary stream beside a data gradient)
    const float* const* params;    // the pass's parameter table (that path's data gradient multiplies the OIHW tensors themselves)
    int br1_on_main = 0;           // conv_wgrad: run the gate branch's generic weight gradient on the main stream (see there)
    int no_join = 0;               // backward pass: leave the auxiliary stream un-joined at the end (mcvc_gen_backward_flags)
    int fuse_next = 0;             // the caller's next step is a norm that can absorb a Winograd output transform (set before conv_fwd)
    const struct WinoFam* pend_fam = nullptr;   // the output transform of this family in `pend` has not run yet -- norm_fwd runs it (fused when it fits)
    WinoOutArgs pend;
    int store_grads = 0;           // backward pass: the weight gradients of the covered layers are STORED (MCVC_BWD_STORE_GRADS; conv_wgrad)
    int force_scheme = 0;          // op-level entries (mcvc_layer_*): 0 planner's choice, 1 Winograd with 2x2 output tiles only, 2 with 4x4 tiles
                                   // (thresholds on samples / tiles lifted), 3 no Winograd, 4 no Winograd and no staged GEMM (direct kernels)
    PackFresh fresh;               // per layer, the forms the last re-pack of `packed` left fresh (never packed through a restricted entry: all)
    unsigned* sync;                // arrival counters of the persistent trunk kernels (MCVC_TRUNK_SYNC_WORDS words of the scratch)
    std::vector<std::pair<const void*, hipEvent_t>> readers;
    void fail(int e) { if (!err && e) err = e; }
};

// What the last re-pack of a packed-weight buffer left fresh: per layer (ConvSpec::index) the mask of forms it refreshed.  The restricted
// entries (mcvc_gen_pack_ranges, the fused updates, mcvc_disc_pack_batch) refresh only the forms their schedule reads; each records the
// very masks it built its job table from (record_fresh), every pass looks its buffer up, and a kernel about to read a form that is not
// fresh fails the pass (stale) or takes the scheme whose sets are (wino4_applies / wino43_applies) instead of reading old weights.
static std::mutex g_pack_mu;
static std::map<const void*, PackFresh> g_pack_fresh;
static PackFresh get_fresh(const void* packed)
{
    std::lock_guard<std::mutex> lk(g_pack_mu);
    auto it = g_pack_fresh.find(packed);
    return it == g_pack_fresh.end() ? PackFresh() : it->second;          // never seen: assume a full pack
}

// small pool of timing-less events, reused round-robin (a backward pass uses a few dozen; the pool is far larger, so an
// event is never re-recorded while a wait on its previous use can still be pending)
static hipEvent_t pool_event()
{
    static std::mutex mu;
    static std::vector<hipEvent_t> pool;
    static size_t next = 0;
    std::lock_guard<std::mutex> lk(mu);
    if (pool.empty()) {            // the whole pool is created on first use (outside any stream capture: the warm-up iterations)
        pool.resize(1024);
        for (hipEvent_t& e : pool) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    }
    next = (next + 1) % pool.size();
    return pool[next];
}

static bool is_fresh(const Exec& ex, const ConvSpec& c, PackForm f) { return (ex.fresh.layer[c.index] >> f & 1) != 0; }
// (a weight gradient reads no weight set; it follows the scheme of the buffer's schedule: the one some layer's fresh sets stand for)
static bool any_fresh(const Exec& ex, PackForm f) { for (unsigned m : ex.fresh.layer) if (m >> f & 1) return true; return false; }
// a kernel is about to read form f of layer c: fail the pass when the last re-pack did not refresh it
static bool stale(Exec& ex, const ConvSpec& c, PackForm f)
{
    if (ex.dry || is_fresh(ex, c, f)) return false;
    ex.fail(MCVC_ERR_INVALID);
    return true;
}

// the main stream is about to overwrite `buf`: wait for aux-stream kernels that still read it
static void wait_readers(Exec& ex, const void* buf)
{
    if (!ex.s2 || ex.dry) return;
    for (auto it = ex.readers.begin(); it != ex.readers.end();) {
        if (it->first == buf) { ex.fail(mcvc_stream_wait(ex.s, it->second)); it = ex.readers.erase(it); }
        else ++it;
    }
}

// the stream for work that runs beside the main chain: the auxiliary stream, made to wait for everything issued on the main stream so far
static hipStream_t fork_aux(Exec& ex)
{
    if (!ex.s2) return ex.s;
    hipEvent_t e = pool_event();
    ex.fail(mcvc_event_record(e, ex.s));
    ex.fail(mcvc_stream_wait(ex.s2, e));
    return ex.s2;
}

static void join_aux(Exec& ex)
{
    if (!ex.s2 || ex.dry) return;
    hipEvent_t e = pool_event();
    ex.fail(mcvc_event_record(e, ex.s2));
    ex.fail(mcvc_stream_wait(ex.s, e));
    ex.readers.clear();
}

// -------------------------------------------------------------------------------------------------
static ConvSpec mk(int Cin, int Cout, int nbr, int KH, int KW, int stride, int ph, int pw, int w0, int b0, int w1, int b1, int bias_grad)
{
    ConvSpec c{};
    c.Cin = Cin; c.Cout = Cout; c.nbr = nbr; c.KH = KH; c.KW = KW; c.stride = stride; c.ph = ph; c.pw = pw;
    c.wi[0] = w0; c.bi[0] = b0; c.wi[1] = w1; c.bi[1] = b1; c.has_bias_grad = bias_grad;
    return c;
}

static inline int conv_out(int H, int K, int s, int p) { return (H + 2 * p - K) / s + 1; }

// ---- conv wrappers ---------------------------------------------------------------------------------
static void run_conv(Exec& ex, const ConvProblem& p, int NB, ConvIO io, long long y_total, const float* w, int w_rows, int w_cout,
                     const float* bias, int allow_split, int force_nsplit, int* nsplit_out)
{
    int ns = 1;
    if (force_nsplit > 0) ns = force_nsplit;
    else if (allow_split) ns = mcvc_conv_plan_nsplit(p, NB, 1);
    if (ns < 1) { ex.fail(MCVC_ERR_INVALID); ns = 1; }
    if (ex.max_split > 0 && ns > ex.max_split) ns = ex.max_split;
    if (io.accumulate && mcvc_deterministic()) ns = 1;          // a K-split accumulate adds with atomics
    if (!io.accumulate) {
        const long long need = (long long)(ns - 1) * y_total;
        if (need > ex.slab_need) ex.slab_need = need;
        if (!ex.dry && need > ex.slab_cap) { ex.fail(MCVC_ERR_WORKSPACE); return; }
    }
    if (nsplit_out) *nsplit_out = io.accumulate ? 1 : ns;
    if (ex.dry) return;
    io.slabs = ex.slabs; io.slab_stride = y_total; io.nsplit = ns;
    ex.fail(mcvc_conv_launch(p, NB, io, w, w_rows, w_cout, bias, ex.s, nullptr));
}

static bool wino_env_enabled()
{
    static const int en = mcvc_knob("MCVC_WINO", 1);
    return en != 0;
}
static thread_local int t_no_wino = 0;          // (op-level entries that ask for the direct / staged-GEMM kernels)
// Precise mode (mcvc_set_precise / env MCVC_PRECISE): every 5x5 layer on the direct kernels -- no Winograd scheme anywhere.  The fast default
// trades rounding for multiplies (after four Adam steps its parameters sit 2-3x further from an fp64 run than the
// reference's own fp32 arithmetic does; precise mode sits where the reference sits).  Process-wide; set it BEFORE networks are packed and
// engines are built (workspaces and packed copies are planned for the mode in force; a later switch fails loudly on a stale copy).
static int g_precise = [] { const char* e = getenv("MCVC_PRECISE"); return (e && atoi(e) != 0) ? 1 : 0; }();
static bool wino_enabled() { return wino_env_enabled() && !t_no_wino && !g_precise; }

// tile of the 36 batched products: 128 channels x 64 tiles measured best on all four shapes (128x128 wastes the ragged
// tile count of upSample1, 256x32 re-reads V too often); knob: MCVC_WINO_CFG = planner index + 1
static int wino_tile_cfg(int M, long long NT)
{
    static const int knob = mcvc_knob("MCVC_WINO_CFG", -1);
    (void)M; (void)NT;
    return knob >= 0 ? knob : 2;
}

// Samples per Winograd pass: the V / M workspaces hold at most kWinoMaxTiles tiles; a larger batch runs in equal chunks of samples
// (every op of the three-launch pipeline is per sample; weight gradients add up over the chunks).  0 = not applicable.
constexpr long long kWinoMaxTiles = 16384;
static int wino_chunk(int NB, long long tiles_per_sample)
{
    if (tiles_per_sample <= 0 || tiles_per_sample > kWinoMaxTiles) return 0;
    const long long nbmax = kWinoMaxTiles / tiles_per_sample;
    if (NB <= nbmax) return NB;
    const long long nch = (NB + nbmax - 1) / nbmax;
    return (int)((NB + nch - 1) / nch);
}
static long long wino_chunk_tiles(int NB, long long tiles_per_sample)          // padded tile count of the largest chunk
{
    const int nbc = wino_chunk(NB, tiles_per_sample);
    return nbc ? ((nbc * tiles_per_sample + 31) & ~31LL) : 0;
}

// 5x5 stride-1 conv as Winograd F(2x2,5x5): input transform -> 36 batched [M x K] x [K x tiles] products (one launch of the
// direct-conv kernel as a 1x1 conv over 36 images with per-image weights) -> output transform (+bias, PixelShuffle store).
// dgrad: the same on the flipped / transposed weight set; K = conv output channels, M = conv input channels.
// F(4x4,5x5) (wino4.h) from `MCVC_WINO4_NB` samples per pass on images whose sides are multiples of 4, when the packed buffer holds the
// 64-point weight sets, fresh: 2.25x fewer multiplies and 2.25x smaller V / M than F(2x2,5x5).  Measured (ms/step, off vs on):
// bs=1 6.77 / 6.64 (upSample2 only: upSample1 has 20 tiles per sample), bs=2 10.8 / 10.3, bs=4 17.5 / 15.1, bs=8 31.1 / 24.3, bs=32 118.1 / 84.5
// (the last three with F(4x4,3x3) on downSample1/2 as well, MCVC_WINO43_NB: at one sample per pass that one costs 0.3 ms)
static int wino4_min_nb()
{
    static const int nb = mcvc_knob("MCVC_WINO4_NB", 1);
    return nb;
}
// fewest F(4x4,5x5) tiles in a pass (the GEMM's column count; 32-column granularity)
static int wino4_min_tiles()
{
    static const int n = mcvc_knob("MCVC_WINO4_MIN_TILES", 64);
    return n < 32 ? 32 : n;
}
static int wino43_min_nb()
{
    static const int nb = mcvc_knob("MCVC_WINO43_NB", 4);
    return nb;
}
static bool wino4_applies(const Exec& ex, const ConvSpec& c, int NB, int H, int W, bool reads_set = true)
{
    if (ex.force_scheme == 1 || ex.force_scheme >= 3) return false;
    if (ex.force_scheme == 2) return c.wino && (H & 3) == 0 && (W & 3) == 0;
    return c.wino && wino4_min_nb() > 0 && NB >= wino4_min_nb() && (H & 3) == 0 && (W & 3) == 0 &&
           (reads_set ? is_fresh(ex, c, PF_W4F) : any_fresh(ex, PF_W4F));
}
// F(4x4,3x3) for the stride-2 5x5 layers in phase form (wino43_kernels.hip) under the same conditions (OH x OW = the conv's output size)
static bool wino43_applies(const Exec& ex, const ConvSpec& c, int NB, int OH, int OW, bool reads_set = true)
{
    if (ex.force_scheme == 1 || ex.force_scheme >= 3) return false;
    if (ex.force_scheme == 2) return c.wino3 && (OH & 3) == 0 && (OW & 3) == 0;
    return c.wino3 && wino43_min_nb() > 0 && NB >= wino43_min_nb() && (OH & 3) == 0 && (OW & 3) == 0 &&
           (reads_set ? is_fresh(ex, c, PF_W43F) : any_fresh(ex, PF_W43F));
}
// samples per F(4x4) pass: V / M hold pts * max(K, M) * tiles floats
static int wino4_chunk(const Exec& ex, int NB, long long tiles_per_sample, int KM, int pts)
{
    const long long cap_tiles = (ex.wino_cap / ((long long)pts * KM)) & ~31LL;
    if (tiles_per_sample <= 0 || cap_tiles < tiles_per_sample) return 0;
    const long long nbmax = cap_tiles / tiles_per_sample;
    if (NB <= nbmax) return NB;
    const long long nch = (NB + nbmax - 1) / nbmax;
    return (int)((NB + nch - 1) / nch);
}

// ---- the four Winograd families ------------------------------------------------------------------------------------------------------------
// What the passes below differ in from family to family.  The phase-form launchers (a stride-2 5x5 layer as a 3x3 convolution over the four
// input phases) take the original image's size on top; the 5x5 families serve one-branch layers, so their dw launcher has no gate tensor.
struct WinoFam {
    int pts;             // transform points: batched products per pass, matrices per weight set
    int nxi;             // ... as WinoGemmArgs::nxi names them (0 = the launcher's default, 36)
    int tile;            // side of an output tile
    int pad;             // padding of the stride-1 convolution
    int min_pitch;       // smallest tile pitch of V / M in a forward / data-gradient pass
    int norm_pts;        // the family's name in mcvc_norm_fwd_wino_applies / _launch (wino.h)
    int (*input)(const WinoXformArgs&, hipStream_t);
    int (*input_phase)(const WinoXformArgs&, int XH, int XW, hipStream_t);
    int (*output)(const WinoOutArgs&, hipStream_t);
    int (*input_t)(const WinoXformArgs&, hipStream_t);                          // the weight gradient's tile-major operands ...
    int (*input_phase_t)(const WinoXformArgs&, int XH, int XW, hipStream_t);
    int (*dy_t)(const WinoXformArgs&, hipStream_t);
    int (*dw)(const float* du, float* dw0, float* dw1, int Cout, int nbr, int Cin, int store, hipStream_t);      // ... and dW (+)= G^T dU G
};
enum { kF23, kF25, kF43, kF45 };          // F(2x2,3x3), F(2x2,5x5), F(4x4,3x3), F(4x4,5x5)
static const WinoFam kWino[4] = {
    {16, 16, 2, 1, 32, 16, mcvc_wino3_input_launch, mcvc_wino3_input_phase_launch, mcvc_wino3_output_launch,
     nullptr, mcvc_wino3_input_phase_t_launch, mcvc_wino3_dy_t_launch, mcvc_wino3_dw_launch},
    {36, 0, 2, 2, 32, 36, mcvc_wino_input_launch, nullptr, mcvc_wino_output_launch,
     mcvc_wino_input_t_launch, nullptr, mcvc_wino_dy_t_launch,
     [](const float* du, float* dw0, float*, int Cout, int, int Cin, int store, hipStream_t s) { return mcvc_wino_dw_launch(du, dw0, Cout, Cin, store, s); }},
    {36, 36, 4, 1, 32, 43, mcvc_wino43_input_launch, mcvc_wino43_input_phase_launch, mcvc_wino43_output_launch,
     nullptr, mcvc_wino43_input_phase_t_launch, mcvc_wino43_dy_t_launch, mcvc_wino43_dw_launch},
    {64, 64, 4, 2, 64 /* (the GEMM wants a pitch of 64+ columns) */, 64, mcvc_wino4_input_launch, nullptr, mcvc_wino4_output_launch,
     mcvc_wino4_input_t_launch, nullptr, mcvc_wino4_dy_t_launch,
     [](const float* du, float* dw0, float*, int Cout, int, int Cin, int store, hipStream_t s) { return mcvc_wino4_dw_launch(du, dw0, Cout, Cin, store, s); }},
};
static long long wino_tiles(const WinoFam& f, int H, int W) { return (long long)((H + f.tile - 1) / f.tile) * ((W + f.tile - 1) / f.tile); }

// Samples per pass of family f over NB samples of `tiles` tiles each and max(K, M) = KM channels; 0 = the family does not apply.
// 4x4 tiles: capacity by wino4_chunk, at least min_tiles real tiles per pass unless the op-level entry forces the scheme.
// 2x2 tiles: the largest chunk's padded tile count fits wino_cap and reaches min_tiles (no exemption).
static int wino_nbc(const Exec& ex, const WinoFam& f, int NB, long long tiles, int KM, int min_tiles)
{
    if (f.tile == 4) {
        const int nbc = wino4_chunk(ex, NB, tiles, KM, f.pts);
        return (nbc && (nbc * tiles >= min_tiles || ex.force_scheme == 2)) ? nbc : 0;
    }
    const int nbc = wino_chunk(NB, tiles);
    const long long NTc = wino_chunk_tiles(NB, tiles);
    return (nbc && NTc >= min_tiles && f.pts * NTc * KM <= ex.wino_cap) ? nbc : 0;
}

// One forward / data-gradient pass, in chunks of nbc samples: input transform -> f.pts batched [M x K] x [K x tiles] products -> output transform.
struct WinoPass {
    const WinoFam* f;
    int K, M;                                           // input / output channels of the stride-1 convolution
    int NB, nbc;
    int H, W;                                           // its image = output size (phase form: the phase planes')
    int XH, XW;                                         // phase form: the original image x addresses; 0 = x is the image itself
    const float* a; long long a_xi; int lda, a_rows;    // weight set U[pts][a_rows (+ pad row)][lda]
    const float* bias;
    int shuffle, YH, YW, accumulate;                    // the store (WinoOutArgs)
    bool may_defer;                                     // the output transform may be left to the next norm_fwd
};
static void wino_pass(Exec& ex, const WinoPass& p, CTensor x, Tensor y)
{
    const WinoFam& f = *p.f;
    const int K = p.K, M = p.M, TH = (p.H + f.tile - 1) / f.tile, TW = (p.W + f.tile - 1) / f.tile;
    for (int b0 = 0; b0 < p.NB; b0 += p.nbc) {
        const int nb = p.NB - b0 < p.nbc ? p.NB - b0 : p.nbc;
        const long long NT = (long long)nb * TH * TW, NTp = std::max<long long>((NT + 31) & ~31LL, f.min_pitch);
        WinoXformArgs xi{};
        xi.x = x.samples(b0, nb).p; xi.x_sb = x.sb; xi.x_sc = x.sc; xi.x_sh = x.sh; xi.v = ex.wv;
        xi.N = nb; xi.C = K; xi.H = p.H; xi.W = p.W; xi.TH = TH; xi.TW = TW; xi.NT = (int)NT; xi.NTp = (int)NTp; xi.pad = f.pad;
        ex.fail(p.XH ? f.input_phase(xi, p.XH, p.XW, ex.s) : f.input(xi, ex.s));
        static const int own_gemm = mcvc_knob("MCVC_WINO_GEMM", 1);
        if (&f != &kWino[kF25] || (own_gemm && (M % 128) == 0 && (K % 16) == 0 && NTp >= 64)) {
            WinoGemmArgs ga{};
            ga.a = p.a; ga.a_xi = p.a_xi; ga.lda = p.lda;
            ga.b = ex.wv; ga.b_xi = (long long)K * NTp; ga.ldb = (int)NTp;
            ga.c = ex.wm; ga.c_xi = (long long)M * NTp; ga.ldc = (int)NTp;
            ga.M = M; ga.N = (int)NTp; ga.K = K; ga.nxi = f.nxi;
            ex.fail(mcvc_wino_gemm_launch(ga, ex.s));
        } else {
            // F(2x2,5x5) outside the GEMM's shapes: one launch of the direct-conv kernel as a 1x1 conv over 36 images with per-image weights;
            // the 36 products see the tiles as a (NTp/32) x 32 "image" so that the conv kernel's 2-D pixel tiles are full
            ConvProblem cp{K, (int)(NTp / 32), 32, M, (int)(NTp / 32), 32, 1, 1, 1, 0, 0};
            ConvIO io = conv_io(nchw(ex.wv, 36, K, (int)(NTp / 32), 32), nchw(ex.wm, 36, M, (int)(NTp / 32), 32));
            io.nsplit = 1;
            io.w_nstride = p.a_xi;
            io.tile_cfg = wino_tile_cfg(M, NT);
            io.gemm_ok = 1;
            ex.fail(mcvc_conv_launch(cp, 36, io, p.a, p.a_rows, p.lda, nullptr, ex.s, nullptr));
        }
        WinoOutArgs oa{};
        oa.m = ex.wm; oa.bias = p.bias;
        oa.y = y.samples(b0, nb).p; oa.y_sb = y.sb; oa.y_sc = y.sc; oa.y_sh = y.sh;
        oa.N = nb; oa.Cout = M; oa.OH = p.H; oa.OW = p.W; oa.TH = TH; oa.TW = TW; oa.NT = (int)NT; oa.NTp = (int)NTp;
        oa.shuffle = p.shuffle; oa.YH = p.YH; oa.YW = p.YW; oa.accumulate = p.accumulate;
        if (p.may_defer && ex.fuse_next && p.nbc == p.NB) { ex.pend = oa; ex.pend_fam = &f; }
        else ex.fail(f.output(oa, ex.s));
    }
}

// One weight-gradient pass on stream ws, in chunks of nbc samples: the tile-major operands Vt[xi][tile][ci] from x and dMt[xi][tile][co] = A dY A^T,
// f.pts products dU[xi] = dMt[xi]^T Vt[xi] over the tiles, then dW += G^T dU G -- the chunks add up in dw (`store`: the FIRST chunk stores its
// gradient instead of adding to what dw held, the later ones add to it).  A stride-2 layer runs in the phase
// formulation (see conv_wino3): dU[xi][co][4ci+2p+q], both branches (value | gate) in one product, the 3x3 blocks scattered back into the two
// 5x5 gradients.
static void wino_wgrad_pass(Exec& ex, const WinoFam& f, const ConvSpec& c, float* const* grads, int nbc, CTensor x, CTensor dy, int store, hipStream_t ws)
{
    const bool phase = c.stride == 2;
    const int NB = x.N, H = x.H, W = x.W;
    const int IH = phase ? H / 2 : H, IW = phase ? W / 2 : W, N = phase ? 4 * c.Cin : c.Cin, M = c.cout_tot;
    const int TH = (IH + f.tile - 1) / f.tile, TW = (IW + f.tile - 1) / f.tile;
    for (int b0 = 0; b0 < NB; b0 += nbc) {
        const int nb = NB - b0 < nbc ? NB - b0 : nbc;
        const long long NT = (long long)nb * TH * TW, NTp = (NT + 31) & ~31LL;
        WinoXformArgs xi{};
        xi.x = x.samples(b0, nb).p; xi.x_sb = x.sb; xi.x_sc = x.sc; xi.x_sh = x.sh; xi.v = ex.wv2;
        xi.N = nb; xi.C = N; xi.H = IH; xi.W = IW; xi.TH = TH; xi.TW = TW; xi.NT = (int)NT; xi.NTp = (int)NTp; xi.pad = f.pad;
        ex.fail(phase ? f.input_phase_t(xi, H, W, ws) : f.input_t(xi, ws));
        WinoXformArgs di{};
        di.x = dy.samples(b0, nb).p; di.x_sb = dy.sb; di.x_sc = dy.sc; di.x_sh = dy.sh; di.v = ex.wm2;
        di.N = nb; di.C = M; di.H = IH; di.W = IW; di.TH = TH; di.TW = TW; di.NT = (int)NT; di.NTp = (int)NTp; di.pad = 0;
        ex.fail(f.dy_t(di, ws));
        WinoGemmArgs ga{};
        ga.a = ex.wm2; ga.a_xi = NTp * M; ga.lda = M;
        ga.b = ex.wv2; ga.b_xi = NTp * N; ga.ldb = N;
        ga.c = ex.wu; ga.c_xi = (long long)M * N; ga.ldc = N;
        // (rows [NT, NTp) of the tile-major operands are zeros: contract over the 16-row stages that hold tiles -- 80 instead of 96 at one sample)
        ga.M = M; ga.N = N; ga.K = (int)((NT + 15) & ~15LL); ga.nxi = f.nxi;
        ex.fail(mcvc_wino_gemm_launch(ga, ws));
        ex.fail(f.dw(ex.wu, grads[c.wi[0]], c.nbr == 2 ? grads[c.wi[1]] : nullptr, c.Cout, c.nbr, c.Cin, store && b0 == 0, ws));
    }
}

// 5x5 stride-1 conv (upSample1/2; see above wino4_min_nb): F(4x4,5x5) where it applies, else F(2x2,5x5)
static bool conv_wino(Exec& ex, const ConvSpec& c, const float* packed, int dgrad, CTensor x, Tensor y, int shuffle, int accumulate)
{
    if (!c.wino || !wino_enabled() || !ex.wv) return false;
    const int NB = x.N, H = dgrad ? y.H : x.H, W = dgrad ? y.W : x.W;          // the convolution's input image: x, or the dX a data gradient writes
    const int K = dgrad ? c.cout_tot : c.Cin, M = dgrad ? c.Cin : c.cout_tot;
    const WinoFam* f = &kWino[kF45];
    int nbc = 0;
    if (wino4_applies(ex, c, NB, H, W) && (M % 128) == 0 && (K % 16) == 0) nbc = wino_nbc(ex, *f, NB, wino_tiles(*f, H, W), K > M ? K : M, wino4_min_tiles());
    if (!nbc) {
        // (gen_pack_cfg skips the 36-point sets of a layer whose EVERY pass at the engine's frame count takes the 4 x 4 scheme; a pass at another
        //  frame count on the same packed buffer that does reach this path reads no stale set: ADVICE r5)
        if (stale(ex, c, wino_form(false, dgrad))) return true;
        f = &kWino[kF25];
        nbc = wino_nbc(ex, *f, NB, wino_tiles(*f, H, W), K > M ? K : M, 0);
    }
    if (!nbc) return false;
    if (ex.dry) return true;
    const bool four = f->tile == 4;
    WinoPass p{};
    p.f = f; p.K = K; p.M = M; p.NB = NB; p.nbc = nbc; p.H = H; p.W = W;
    const PackForm form = wino_form(four, dgrad);
    p.a = packed + c.off[form]; p.a_xi = form_xi(c, form); p.lda = kPackForms[form].ld(c); p.a_rows = dgrad ? c.dg_rows_co : c.cin_pad;
    p.bias = dgrad ? nullptr : packed + c.off[PF_BIAS];
    p.shuffle = shuffle; p.YH = 2 * H; p.YW = 2 * W; p.accumulate = accumulate;
    p.may_defer = !dgrad && shuffle;
    wino_pass(ex, p, x, y);
    return true;
}

// 5x5 stride-2 padding-2 conv (downSample1/2) as a 3x3 stride-1 conv: F(4x4,3x3) (36 points per 16 outputs) where it applies, else F(2x2,3x3).
// Forward (H, W even): over the four input phases, K = 4*Cin.  dgrad: the merged data gradient = a conv over dY with 4*Cin output channels and a
// PixelShuffle store into dX; x is dY and y is dX there.  (c.wino3 says 4*Cin % 128 == 0 and cout_tot % 16 == 0: the GEMM's shapes hold for
// the data gradient; these layers' OH x OW is ceil(H/2) x ceil(W/2), what the merged form stores.)
static bool conv_wino3(Exec& ex, const ConvSpec& c, const float* packed, int dgrad, CTensor x, Tensor y, int accumulate)
{
    if (!c.wino3 || !wino_enabled() || !ex.wv) return false;
    const int NB = x.N, H = dgrad ? y.H : x.H, W = dgrad ? y.W : x.W;
    if (!dgrad && ((H & 1) != 0 || (W & 1) != 0 || (c.cout_tot % 128) != 0)) return false;
    static const int en[2] = {mcvc_knob("MCVC_WINO3_FWD", 1), mcvc_knob("MCVC_WINO3", 1)};
    if (!en[dgrad]) return false;
    const int OH = conv_out(H, c.KH, c.stride, c.ph), OW = conv_out(W, c.KW, c.stride, c.pw);
    const int K = dgrad ? c.cout_tot : 4 * c.Cin, M = dgrad ? 4 * c.Cin : c.cout_tot;
    const WinoFam* f = &kWino[kF43];
    int nbc = 0;
    if (wino43_applies(ex, c, NB, OH, OW) && 2 * OH == H && 2 * OW == W) nbc = wino_nbc(ex, *f, NB, wino_tiles(*f, OH, OW), K > M ? K : M, 64);
    if (!nbc) {
        f = &kWino[kF23];
        nbc = wino_nbc(ex, *f, NB, wino_tiles(*f, OH, OW), K > M ? K : M, 64);
    }
    if (!nbc) return false;
    if (ex.dry) return true;
    const bool four = f->tile == 4;
    WinoPass p{};
    p.f = f; p.K = K; p.M = M; p.NB = NB; p.nbc = nbc; p.H = OH; p.W = OW;
    const PackForm form = wino3_form(four, dgrad);
    p.a = packed + c.off[form]; p.a_xi = form_xi(c, form); p.lda = kPackForms[form].ld(c);
    if (dgrad) {
        p.shuffle = 1; p.YH = H; p.YW = W; p.accumulate = accumulate;
    } else {
        p.XH = H; p.XW = W;
        p.bias = packed + c.off[PF_BIAS];
        p.YH = OH; p.YW = OW;
        p.may_defer = true;
    }
    wino_pass(ex, p, x, y);
    return true;
}

// Convolutions that run as staged GEMMs on the LDS-DMA GEMM pipeline (sgemm.h): 1 x KW stride 1 (KW = 1, 3) over an image of rows -- the 1-D
// trunk beyond the fused small-batch kernels (more than 64 columns; MCVC_SGEMM1D_COLS = smallest column count, 0 = never).  (kind 1 of r2-r4,
// the discriminators' 3 x 3 stride-2 layers as staged products -- tap planes, transposed operands, gather -- is gone: those layers run as
// IMPLICIT GEMMs in every pass whose shapes allow it (igemm_applies) and on the direct kernels otherwise.)
struct SgKind { int kind, taps, OH, OW; };
static thread_local int t_no_sgemm = 0;
// (op-level entries: operands are the CALLER's tensors.  The 1 x 3 implicit forms read one float in front of / behind a tensor -- the shifted
//  windows' first / last piece, whose out-of-row element is then dropped -- which is inside the library's own stash / scratch layouts but not
//  guaranteed to be mapped for a foreign allocation: those entries keep the direct kernels for 1-D layers)
static thread_local int t_user_operands = 0;
static SgKind sgemm_kind(const ConvSpec& c, int NB, int H, int W)
{
    static const int min_cols = mcvc_knob("MCVC_SGEMM1D_COLS", 64);
    SgKind k{0, 0, 0, 0};
    if (t_no_sgemm || t_user_operands) return k;
    if (c.nbr > 2 || (c.cout_tot % 64) != 0 || (c.Cout % 32) != 0 || c.cin_pad != c.Cin) return k;
    if (c.KH == 1 && (c.KW == 1 || c.KW == 3) && c.stride == 1 && c.ph == 0 && c.pw == (c.KW - 1) / 2) {
        k.OH = H; k.OW = W; k.taps = c.KW;
        if (min_cols > 0 && (long long)NB * H * W >= min_cols && (c.Cin % 64) == 0 && (W & 3) == 0) k.kind = 2;
    }
    return k;
}
// K-split: the smallest power-of-two split (<= 8) that yields >= 256 workgroups while a slab keeps >= 64 k per half.  (A cost-model split
// against round quantisation -- stream-K's effect with uniform splits -- was built in r4 and measured SLOWER inside the concurrent lanes: bs=8
// 22.2-22.6 -> 23.0-23.2 ms, the other lanes' kernels already fill a product's last round; removed)
static int split_by_cost(long long tiles, int Kmin)
{
    static const int wgs = mcvc_knob("MCVC_SGEMM_WGS", 256);
    static const int maxsp = mcvc_knob("MCVC_SGEMM_MAXSPLIT", 8);
    int sp = 1;
    while (sp < maxsp && tiles * sp < wgs && (Kmin % (64 * sp)) == 0 && Kmin / (2 * sp) >= 64) sp *= 2;
    return sp;
}
static int sgemm_split(int M, long long N, int K)
{
    return split_by_cost((long long)(M / 64) * ((N + 63) / 64), K);
}

// ---- implicit GEMM for the 3x3 stride-2 padding-1 layers (sgemm.h): no tap planes, no gather kernel -------------------------------------
static bool igemm_enabled()
{
    static const int en = mcvc_knob("MCVC_IGEMM", 1);
    return en != 0;
}
static bool igemm_applies(const ConvSpec& c, int H, int W)
{
    return igemm_enabled() && c.igemm && (H & 1) == 0 && (W & 1) == 0 && ((W / 2) & 3) == 0 && H >= 2 && W >= 8;
}
// where the nine taps of such a layer start in its input's phase-split padded layout: tap (kh, kw) of output (oh, ow) reads x[2 oh + kh - 1][2 ow + kw - 1]
static void xs_tap_offsets(int H, int W, long long boff[9])
{
    const int pw = mcvc_xs_pw(W);
    const long long plane = mcvc_xs_plane(H, W);
    for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 3; ++kw) {
            const int ph = (kh == 1) ? 0 : 1, di = (kh == 0) ? -1 : 0, pq = (kw == 1) ? 0 : 1, dj = (kw == 0) ? -1 : 0;
            boff[3 * kh + kw] = (long long)(2 * ph + pq) * plane + (long long)(1 + di) * pw + 4 + dj;
        }
}
// K split: enough 64 x 64 tiles x classes x splits to occupy the chip, at least two 32-deep stages per split of the shortest class
static int igemm_split(long long tiles, int Kmin) { return split_by_cost(tiles, Kmin); }
// forward: xs = the input in the phase-split padded layout, y = the conv output (dense planes); K-split slabs 1.. are summed by the consumer
static void conv_fwd_igemm(Exec& ex, const ConvSpec& c, const float* packed, CTensor xs, Tensor y, int allow_split, int* nsplit)
{
    const int NB = xs.N, H = xs.H, W = xs.W;
    const int OH = H / 2, OW = W / 2, P = OH * OW, KT = 9 * c.Cin;
    const long long NT = (long long)NB * P;
    const int sp = (allow_split && nsplit) ? igemm_split((long long)(c.cout_tot / 64) * ((NT + 63) / 64), KT) : 1;
    const long long slab_need = (long long)(sp - 1) * y.dense();
    if (slab_need > ex.slab_need) ex.slab_need = slab_need;
    if (nsplit) *nsplit = sp;
    if (ex.dry) return;
    if (slab_need > ex.slab_cap) { ex.fail(MCVC_ERR_WORKSPACE); return; }
    const int pw = mcvc_xs_pw(W);
    const long long plane = mcvc_xs_plane(H, W);
    IGemmArgs g{};
    g.ncls = 1;
    g.cls[0].a = packed + c.off[PF_IFWD]; g.cls[0].ntaps = 9; g.cls[0].coff = 0;
    xs_tap_offsets(H, W, g.cls[0].boff);
    for (int t = 0; t < 9; ++t) g.cls[0].aoff[t] = (long long)t * c.Cin * c.cout_pk;      // tap-major copy: rows (tap, ci)
    g.a_ks = c.cout_pk;
    g.b = xs.p; g.b_cs = 4 * plane; g.b_sn = (long long)c.Cin * 4 * plane; g.b_pitch = pw; g.Cb = c.Cin; g.OW = OW; g.P = P;
    g.c = y.p; g.ldc = y.sc; g.c_sn = y.sb; g.c_sh = y.sh; g.c_sw = 1;
    g.bias = packed + c.off[PF_BIAS];
    g.M = c.cout_tot; g.N = (int)NT; g.nsplit = sp; g.c_slab = ex.slabs; g.c_split = y.dense();
    ex.fail(mcvc_igemm_launch(g, ex.s));
}
// data gradient: dyp = dY in the padded layout (planes of (OH + 1) x (OW + 4), zero borders), dx dense; the four output-parity classes in
// one launch, every input pixel written by exactly one of them; K-split slabs (dx-shaped) are summed by the consumer
static void conv_dgrad_igemm(Exec& ex, const ConvSpec& c, const float* packed, CTensor dyp, Tensor dx, int accumulate, int allow_split, int* nsplit)
{
    const int NB = dx.N, H = dx.H, W = dx.W;
    const int OH = H / 2, OW = W / 2, P = OH * OW;
    const long long NT = (long long)NB * P;
    int sp = (allow_split && nsplit && !accumulate) ? igemm_split(4LL * (c.Cin / 64) * ((NT + 63) / 64), c.cout_tot) : 1;
    // (Tried on top, r5: deeper uniform splits -- 4-tap class at most 512 deep -- and tap-wise splits with zero-filled slabs for the classes with
    //  fewer taps, so that every workgroup is one tap deep: bs=1 6.01 -> 6.03-6.12 and -> 6.3 ms.  The consumer reading 4-8 slabs costs more
    //  than the imbalance of the classes; the uniform split of r4 stays.)
    const long long slab_need = (long long)(sp - 1) * dx.dense();
    if (slab_need > ex.slab_need) ex.slab_need = slab_need;
    if (nsplit) *nsplit = sp;
    if (ex.dry) return;
    if (slab_need > ex.slab_cap) { ex.fail(MCVC_ERR_WORKSPACE); return; }
    const int pitch = mcvc_dyp_pitch(OW);
    const long long plane = mcvc_dyp_plane(OH, OW);
    IGemmArgs g{};
    g.ncls = c.ncls;
    for (int k = 0; k < c.ncls; ++k) {
        const DgradClass& d = c.icls[k];
        IGemmClass& q = g.cls[k];
        q.a = packed + c.off[PF_IFWD]; q.ntaps = d.nth * d.ntw;          // the tap-major FORWARD copy, read row-major (sgemm.h arow)
        q.coff = (long long)d.qh * dx.sh + d.qw;
        for (int u = 0; u < d.nth; ++u)
            for (int v = 0; v < d.ntw; ++v) {     // input row 2a + qh receives tap kh from output row a + (qh + 1 - kh) / 2
                const int kh = d.khmax - 2 * u, kw = d.kwmax - 2 * v;
                q.boff[u * d.ntw + v] = (long long)((d.qh + 1 - kh) / 2) * pitch + (d.qw + 1 - kw) / 2;
                q.aoff[u * d.ntw + v] = (long long)(3 * kh + kw) * c.Cin * c.cout_pk;
            }
    }
    g.a_ks = c.cout_pk; g.arow = 1;
    g.b = dyp.p; g.b_cs = plane; g.b_sn = (long long)c.cout_tot * plane; g.b_pitch = pitch; g.Cb = c.cout_tot; g.OW = OW; g.P = P;
    g.c = dx.p; g.ldc = dx.sc; g.c_sn = dx.sb; g.c_sh = 2 * dx.sh; g.c_sw = 2; g.accumulate = accumulate;
    g.M = c.Cin; g.N = (int)NT; g.nsplit = sp; g.c_slab = ex.slabs; g.c_split = dx.dense();
    ex.fail(mcvc_igemm_launch(g, ex.s));
}

static void conv_fwd(Exec& ex, const ConvSpec& c, const float* packed, CTensor x, Tensor y, int shuffle, int allow_split, int* nsplit)
{
    const int NB = x.N, H = x.H, W = x.W;          // (y describes the buffer as stored: behind a PixelShuffle, C / 4 channels of 2H x 2W)
    const SgKind sk = shuffle ? SgKind{0, 0, 0, 0} : sgemm_kind(c, NB, H, W);
    if (sk.kind) {
        const int P = sk.OH * sk.OW, KT = sk.taps * c.Cin;
        const long long NT = (long long)NB * P;
        const bool b_in_place = c.KW == 1;                                                    // a 1x1 conv multiplies x itself
        const int sp = (allow_split && nsplit) ? sgemm_split(c.cout_tot, NT, KT) : 1;       // slabs 1.. are summed by the consumer (norm / act)
        const long long slab_need = (long long)(sp - 1) * y.dense();
        if (ex.dry) { if (slab_need > ex.slab_need) ex.slab_need = slab_need; if (nsplit) *nsplit = sp; return; }
        if (stale(ex, c, PF_FWD)) return;
        if (!b_in_place && slab_need <= ex.slab_cap && y.sh == sk.OW && y.sc == P && (NB == 1 || y.sb == (long long)c.cout_tot * P)) {
            // 1 x 3 over dense rows: an implicit GEMM (sgemm.h) -- the three windows of x are gathered where they lie, shifted by -1 / 0 / +1
            // column; the K-major forward copy's rows are (ci, kw), so a tap's rows are KW apart
            IGemmArgs g{};
            g.ncls = 1;
            IGemmClass& q = g.cls[0];
            q.a = packed + c.off[PF_FWD]; q.ntaps = c.KW; q.coff = 0;
            for (int kw = 0; kw < c.KW; ++kw) { q.boff[kw] = kw - c.pw; q.aoff[kw] = (long long)kw * c.cout_pk; q.zs[kw] = kw < c.pw ? 1 : (kw > c.pw ? 2 : 0); }
            g.a_ks = (long long)c.KW * c.cout_pk; g.zw = W;
            g.b = x.p; g.b_cs = x.sc; g.b_sn = x.sb; g.b_pitch = x.sh; g.Cb = c.Cin; g.OW = W; g.P = P;
            g.c = y.p; g.ldc = y.sc; g.c_sn = y.sb; g.c_sh = y.sh; g.c_sw = 1;
            g.bias = packed + c.off[PF_BIAS];
            g.M = c.cout_tot; g.N = (int)NT; g.nsplit = sp; g.c_slab = ex.slabs; g.c_split = y.dense();
            ex.fail(mcvc_igemm_launch(g, ex.s));
            if (nsplit) *nsplit = sp;
            return;
        }
        if (b_in_place && x.sh == W && x.sc == P && slab_need <= ex.slab_cap && y.sh == sk.OW && y.sc == P &&
            (NB == 1 || y.sb == (long long)c.cout_tot * P)) {
            SGemmArgs g{};
            g.a = packed + c.off[PF_FWD]; g.lda = c.cout_pk;                       // Wt[k = ci][co] (value | gate columns)
            g.b = x.p; g.ldb = x.sc; g.bseg = P; g.b_sn = x.sb;
            g.c = y.p; g.ldc = y.sc; g.cseg = P; g.c_sn = y.sb;
            g.bias = packed + c.off[PF_BIAS];
            g.M = c.cout_tot; g.N = (int)NT; g.K = KT; g.nsplit = sp; g.c_slab = ex.slabs; g.c_split = y.dense();
            ex.fail(mcvc_sgemm_launch(g, ex.s));
            if (nsplit) *nsplit = sp;
            return;
        }
    }
    if (conv_wino(ex, c, packed, 0, x, y, shuffle, 0) || (!shuffle && conv_wino3(ex, c, packed, 0, x, y, 0))) { if (nsplit) *nsplit = 1; return; }
    if (stale(ex, c, PF_FWD)) return;          // the direct kernels are next
    ConvProblem p{c.Cin, H, W, c.cout_tot, conv_out(H, c.KH, c.stride, c.ph), conv_out(W, c.KW, c.stride, c.pw),
                  c.KH, c.KW, c.stride, c.ph, c.pw};
    ConvIO io = conv_io(x, y);
    io.shuffle = shuffle;
    run_conv(ex, p, NB, io, y.dense(), packed + c.off[PF_FWD], c.w_rows, c.cout_pk, packed + c.off[PF_BIAS], allow_split, 0, nsplit);
}

// dX = conv-backward-data.  dy: conv-output layout (cout_tot channels, OHxOW); dx: input layout.
static void conv_dgrad(Exec& ex, const ConvSpec& c, const float* packed, CTensor dy, Tensor dx, int accumulate, int allow_split, int* nsplit)
{
    const int NB = dx.N, H = dx.H, W = dx.W;
    if (conv_wino(ex, c, packed, 1, dy, dx, 0, accumulate)) { if (nsplit) *nsplit = 1; return; }
    const int OH = conv_out(H, c.KH, c.stride, c.ph), OW = conv_out(W, c.KW, c.stride, c.pw);
    const int st = c.stride;
    const SgKind sk = sgemm_kind(c, NB, H, W);
    if (sk.kind) {
        // 1 x KW over dense rows as an implicit GEMM (sgemm.h): M = input channels, K = (kw, output channel); A = the K-major FORWARD copy read
        // row-major (rows (ci, kw), output channels contiguous: arow), B = the windows of dY shifted by pw - kw columns.  An accumulating
        // destination with a K split leaves dx alone: all splits go to slabs and the consumer sums dx + slabs (*nsplit = splits + 1).
        const int P = sk.OH * sk.OW;
        const long long NT = (long long)NB * P;
        int sp = (allow_split && nsplit) ? igemm_split((long long)(c.Cin / 64) * ((NT + 63) / 64), sk.taps * c.cout_tot) : 1;
        while (sp > 1 && ((long long)sk.taps * c.cout_tot) % (32LL * sp) != 0) sp /= 2;
        const bool slab_all = accumulate && sp > 1;
        const long long slab_need = (long long)(slab_all ? sp : sp - 1) * dx.dense();
        if (slab_need > ex.slab_need) ex.slab_need = slab_need;
        if (nsplit) *nsplit = slab_all ? sp + 1 : sp;
        if (ex.dry) return;
        if (stale(ex, c, PF_FWD)) return;
        if (slab_need > ex.slab_cap) { ex.fail(MCVC_ERR_WORKSPACE); return; }
        IGemmArgs g{};
        g.ncls = 1;
        IGemmClass& q = g.cls[0];
        q.a = packed + c.off[PF_FWD]; q.ntaps = c.KW; q.coff = 0;
        for (int kw = 0; kw < c.KW; ++kw) {
            const int sh = c.pw - kw;                 // dX[n] += W[:, :, kw]^T dY[n + pw - kw]
            q.boff[kw] = sh; q.aoff[kw] = (long long)kw * c.cout_pk; q.zs[kw] = sh < 0 ? 1 : (sh > 0 ? 2 : 0);
        }
        g.a_ks = (long long)c.KW * c.cout_pk; g.arow = 1; g.zw = W;
        g.b = dy.p; g.b_cs = dy.sc; g.b_sn = dy.sb; g.b_pitch = dy.sh; g.Cb = c.cout_tot; g.OW = W; g.P = P;
        g.ldc = dx.sc; g.c_sn = dx.sb; g.c_sh = dx.sh; g.c_sw = 1;
        g.M = c.Cin; g.N = (int)NT; g.nsplit = sp; g.c_split = dx.dense();
        if (slab_all) { g.c = ex.slabs; g.c_slab = ex.slabs + dx.dense(); }
        else { g.c = dx.p; g.c_slab = ex.slabs; g.accumulate = accumulate; }
        ex.fail(mcvc_igemm_launch(g, ex.s));
        return;
    }
    if (conv_wino3(ex, c, packed, 1, dy, dx, accumulate)) { if (nsplit) *nsplit = 1; return; }
    static const int ucls_nb = mcvc_knob("MCVC_DGRAD_CLASSES_NB", 8);
    const bool per_class = c.merged && c.off[PF_DCLS] >= 0 && NB >= ucls_nb;
    if (stale(ex, c, per_class ? PF_DCLS : PF_DGRAD)) return;          // the direct kernels are next
    if (c.merged && !per_class) {
        ConvProblem p{c.cout_tot, OH, OW, 4 * c.Cin, (H + 1) / 2, (W + 1) / 2, c.mg_kh, c.mg_kw, 1, c.mg_pad_h, c.mg_pad_w};
        ConvIO io = conv_io(dy, dx);
        io.accumulate = accumulate; io.shuffle = 1; io.YH = H; io.YW = W;
        run_conv(ex, p, NB, io, dx.dense(), packed + c.off[PF_DGRAD], c.dg_rows_co * c.mg_kh * c.mg_kw, c.mg_ld, nullptr, allow_split, 0, nsplit);
        return;
    }
    const DgradClass* klass = per_class ? c.ucls : c.cls;
    const long long kbase = c.off[per_class ? PF_DCLS : PF_DGRAD];
    ConvProblem ps[4];
    int force = 0;
    for (int k = 0; k < c.ncls; ++k) {
        const DgradClass& d = klass[k];
        ps[k] = ConvProblem{c.cout_tot, OH, OW, c.Cin, (H - d.qh + st - 1) / st, (W - d.qw + st - 1) / st,
                            d.nth, d.ntw, 1, d.pad_h, d.pad_w};
    }
    if (c.ncls > 1 && allow_split) {          // all parity classes must agree on the slab count
        force = 1 << 30;
        for (int k = 0; k < c.ncls; ++k) { const int n = mcvc_conv_plan_nsplit(ps[k], NB, 1); if (n < force) force = n; }
        if (force < 1) force = 1;
        if (ex.max_split > 0 && force > ex.max_split) force = ex.max_split;
    }
    int ns_all = 1;
    for (int k = 0; k < c.ncls; ++k) {
        const DgradClass& d = klass[k];
        if (ps[k].OH <= 0 || ps[k].OW <= 0) continue;
        ConvIO io = conv_io(dy, dx);
        io.y = dx.p + (long long)d.qh * dx.sh + d.qw; io.y_sh = dx.sh * st; io.y_sw = st;
        io.accumulate = accumulate;
        int ns = 1;
        // slabs of class k live at the same slab base + the class's element offset
        Exec sub = ex;
        if (!ex.dry) sub.slabs = ex.slabs + (long long)d.qh * dx.sh + d.qw;
        run_conv(sub, ps[k], NB, io, dx.dense(), packed + kbase + d.offset, c.dg_rows_co * d.nth * d.ntw, c.cin_pk, nullptr,
                 allow_split, force, &ns);
        ex.err = sub.err; ex.slab_need = sub.slab_need;
        if (ns > ns_all) ns_all = ns;
    }
    if (nsplit) *nsplit = ns_all;
}

static int wgrad_cin1_enabled()
{
    static const int en = mcvc_knob("MCVC_WGRAD_CIN1", 1);
    return en;
}

// Store mode (ex.store_grads, a covered layer: grad_store_covered): on return the layer's weight gradients EQUAL this pass's, whatever the
// buffer held.  The writers that can store do (the first one of a pass that runs in chunks / slabs; the rest add to it); in front of a
// writer that can only add -- the direct kernel with slabs or atomics, a fall-back at an odd frame count or without a workspace -- the
// tensor is zero-filled on the writer's stream.  So correctness never depends on which writer the planner picks, only the speed does.
static void conv_wgrad(Exec& ex, const ConvSpec& c, float* const* grads, CTensor x, CTensor dy)
{
    const int NB = x.N, H = x.H, W = x.W;
    const int OH = conv_out(H, c.KH, c.stride, c.ph), OW = conv_out(W, c.KW, c.stride, c.pw);
    ConvProblem p{c.Cin, H, W, c.Cout, OH, OW, c.KH, c.KW, c.stride, c.ph, c.pw};
    // GEMM form (sgemm.h): pixel-major operands in the weight gradients' own staging region, K-split slabs, then dw += slabs
    const SgKind sk = sgemm_kind(c, NB, H, W);                            // (the 1 x KW layers of the wide trunk)
    const bool ig3 = x.lay == L_PHASE_SPLIT && igemm_applies(c, H, W);             // a 3 x 3 stride-2 layer whose input arrives phase-split
    const int wtaps = ig3 ? 9 : sk.taps;
    const int KT = wtaps * c.Cin;
    long long sg_floats = 0;
    // implicit form (r5, wgemm_kernels.hip): x arrives phase-split (the layer's forward ran as an implicit GEMM) -- both operands are read where
    // they lie; K split over the pixels when 128 x 32-filter tiles alone cannot fill the chip (slabs in the same staging region, dw_accum sums)
    static const int wgemm_on = mcvc_knob("MCVC_WGEMM", 1);
    const bool implicit = wgemm_on && (ig3 || sk.kind == 2) && (c.cout_tot % 128) == 0 && (c.Cin % mcvc_wgemm_cib(wtaps)) == 0 &&
                          (c.nbr == 1 || (c.Cout % 32) == 0);
    int wg_split = 1;
    if (implicit) {
        const int tiles = (c.cout_tot / 128) * (c.Cin / mcvc_wgemm_cib(wtaps));
        const long long nst = ((long long)NB * OH * OW + 31) / 32;
        static const int wg_target = mcvc_knob("MCVC_WGEMM_WGS", 128), wg_max = mcvc_knob("MCVC_WGEMM_MAXSPLIT", 64);
        // (a workgroup per compute unit -- a tile holds 156 KB of LDS -- and at least two pixel stages per split.  The target is 128 per
        // NETWORK: a grouped pass (twin.h) launches both networks' tiles in one grid, and at 256 per network that grid ran two rounds on
        // 256 CUs while dw_accum summed twice the slabs -- bs=1 step 5.70 -> 5.60 ms at 128.  The ungrouped passes plan the same split,
        // so the grouped step stays bit-identical to the four-lane one.)
        while (wg_split < wg_max && tiles * wg_split < wg_target && nst / (2 * wg_split) >= 2) wg_split *= 2;
        sg_floats = wg_split > 1 ? (long long)wg_split * c.cout_tot * KT : 0;
    }
    if (ex.dry) {          // K-split slabs: their own region, so they never alias the data-gradient slabs of the main stream
        if (implicit && sg_floats > ex.sgw_need) ex.sgw_need = sg_floats;          // (the direct kernel's slabs stay reserved as the fallback)
        const long long need = mcvc_wgrad_plan_slab_floats(p, NB);
        if (need > ex.wslab_need) ex.wslab_need = need;
        return;
    }
    if (!grads) return;
    hipStream_t ws = fork_aux(ex);           // dY (and x) are complete on the main stream at this point
    const bool store = ex.store_grads && grad_store_covered(c);
    const long long wnumel = (long long)c.Cout * c.Cin * c.KH * c.KW;
    auto zero_fill = [&](int br, hipStream_t zs) {            // store mode in front of a writer that can only add
        if (store && grads[c.wi[br]]) ex.fail(mcvc_zero_words_launch(grads[c.wi[br]], wnumel, zs));
    };
    bool done = false;
    if (implicit && (wg_split == 1 || (ex.sgw && sg_floats <= ex.sgw_cap)) && grads[c.wi[0]] && (c.nbr == 1 || grads[c.wi[1]])) {
        WGemmArgs g{};
        g.a = dy.p; g.a_cs = dy.sc; g.a_sn = dy.sb; g.a_pitch = dy.sh;
        g.b = x.p; g.b_cs = x.sc; g.b_sn = x.sb; g.ntaps = wtaps;
        if (ig3) {
            g.b_pitch = mcvc_xs_pw(W);
            xs_tap_offsets(H, W, g.boff);
        } else {                                          // 1 x KW over dense rows: tap kw multiplies x[w + kw - pw]; the rows' ends count as padding
            g.b_pitch = x.sh; g.zw = (c.KW == 3) ? W : 0;
            for (int kw = 0; kw < c.KW; ++kw) g.boff[kw] = kw - c.pw;
        }
        g.OW = OW; g.P = OH * OW; g.NPIX = NB * g.P;
        g.M = c.cout_tot; g.Cin = c.Cin; g.nsplit = wg_split;
        if (wg_split == 1) {
            g.c = grads[c.wi[0]]; g.accumulate = store ? 0 : 1;
            if (c.nbr == 2) { g.c2 = grads[c.wi[1]]; g.m_split = c.Cout; }
            ex.fail(mcvc_wgemm_launch(g, ws));
        } else {
            g.c = ex.sgw; g.c_split = (long long)c.cout_tot * KT; g.c_slab = ex.sgw + g.c_split;
            ex.fail(mcvc_wgemm_launch(g, ws));
            ex.fail(mcvc_dw_accum_launch(ex.sgw, wg_split, g.c_split, grads[c.wi[0]], c.nbr == 2 ? grads[c.wi[1]] : nullptr, c.Cout, c.cout_tot, KT, ws, store));
        }
        done = true;
    }
    if (!done && x.lay == L_PHASE_SPLIT) { ex.fail(MCVC_ERR_WORKSPACE); return; }     // (nothing else reads a phase-split input: never fall through to a dense reader)
    if (!done && (c.wino ? c.nbr == 1 : c.wino3 && (H & 1) == 0 && (W & 1) == 0 && (c.nbr == 1 || grads[c.wi[1]])) && wino_enabled() && ex.wu && grads[c.wi[0]]) {
        // Winograd weight gradient (wino_wgrad_pass); the stride-2 layers' 3x3 convolution runs over the phase planes, OH x OW
        static const int en25 = mcvc_knob("MCVC_WINO_WGRAD", 1), en3 = mcvc_knob("MCVC_WINO3_WGRAD", 1);
        const int IH = c.wino ? H : OH, IW = c.wino ? W : OW, N = c.wino ? c.Cin : 4 * c.Cin, M = c.cout_tot;
        auto attempt = [&](const WinoFam& f, int en, int min_tiles) {
            if (!en || (M % 128) != 0 || (N % 64) != 0 || (long long)f.pts * M * N > ex.wu_cap) return false;
            const int nbc = wino_nbc(ex, f, NB, wino_tiles(f, IH, IW), M > N ? M : N, min_tiles);
            if (nbc) wino_wgrad_pass(ex, f, c, grads, nbc, x, dy, store, ws);
            return nbc != 0;
        };
        // (MCVC_WINO_WGRAD switches the 36-point form only)
        if (c.wino) done = (wino4_applies(ex, c, NB, H, W, false) && attempt(kWino[kF45], 1, 32)) || attempt(kWino[kF25], en25, 0);
        else done = (wino43_applies(ex, c, NB, OH, OW, false) && attempt(kWino[kF43], en3, 32)) || attempt(kWino[kF23], en3, 0);
    }
    if (!done && c.cout_tot == 1 && mcvc_wgrad_cout1_applies(p) && grads[c.wi[0]]) {       // one output channel: VALU kernel
        WgradIO io{x.p, x.sb, x.sc, x.sh, dy.p, dy.sb, dy.sc, dy.sh};
        ex.fail(mcvc_wgrad_cout1_launch(p, NB, io, grads[c.wi[0]], ws));          // (an edge layer: never covered, always adds)
        done = true;
    }
    for (int br = 0; br < c.nbr && !done; ++br) {
        float* dw = grads[c.wi[br]];
        if (!dw) continue;
        WgradIO io{x.p, x.sb, x.sc, x.sh, dy.p + (long long)br * c.Cout * dy.sc, dy.sb, dy.sc, dy.sh};
        if (mcvc_wgrad_cin1_applies(p) && wgrad_cin1_enabled()) { ex.fail(mcvc_wgrad_cin1_launch(p, NB, io, dw, ws)); continue; }      // (edge layers, like cin2 below)
        // last layer of a backward pass with nothing left for the main stream (conv1 without an input gradient): the gate branch runs
        // there, beside the value branch on the auxiliary stream (atomic accumulation into its own tensor, no slabs to share)
        const bool on_main = br == 1 && ex.br1_on_main && ex.s2 && !mcvc_deterministic() && (long long)c.Cout * c.Cin * c.KH * c.KW <= 65536;
        if (mcvc_wgrad_cin2_applies(p, io)) { ex.fail(mcvc_wgrad_cin2_launch(p, NB, io, dw, on_main ? ex.s : ws)); continue; }
        const bool sk_store = store && mcvc_wgrad_smallk_applies(p, NB);          // (the small-K kernel stores; the slab / atomic kernels only add)
        if (!sk_store) zero_fill(br, on_main ? ex.s : ws);
        ex.fail(mcvc_wgrad_launch(p, NB, io, dw, ex.wslabs, ex.wslab_cap, on_main ? ex.s : ws, sk_store));
    }
    if (ex.s2) {
        hipEvent_t e = pool_event();
        ex.fail(mcvc_event_record(e, ex.s2));
        ex.readers.emplace_back((const void*)dy.p, e);
    }
}

static void conv_bias_grad(Exec& ex, const ConvSpec& c, float* const* grads, CTensor dy)
{
    const int NB = dy.N, P = dy.P();
    if (ex.dry || !grads || !c.has_bias_grad) return;
    for (int br = 0; br < c.nbr; ++br) {
        float* db = grads[c.bi[br]];
        if (!db) continue;
        ex.fail(mcvc_bias_grad_launch(dy.p + (long long)br * c.Cout * dy.sc, dy.sb, dy.sc, NB, c.Cout, P, db, ex.s));
    }
}

// ---- whole-network pack: job tables (packforms.h) built once per plan, resident on the device ---------------------
// A plan: which forms of which layers of which network a table refreshes, in table order.  It is the cache key of the device tables -- a
// comparable VALUE, so two different plans never share a table -- and what the staleness records are set from.
struct PackPlan {
    int dev = 0, net = 0, update = 0;                  // net: 0 generator, 1 discriminator, 2 one op-level layer of `shape`
    int sets = 3;                                      // 1: the forms a forward pass reads, 2: those only a backward pass reads, 3: both
    std::array<int, 8> shape{};
    std::vector<std::pair<int, unsigned>> layers;      // (ConvSpec::index, forms)
    void add(const ConvSpec& c, unsigned forms) { layers.emplace_back(c.index, forms & spec_forms(c)); }
    bool operator<(const PackPlan& o) const
    { return std::tie(dev, net, update, sets, shape, layers) < std::tie(o.dev, o.net, o.update, o.sets, o.shape, o.layers); }
};
static PackTable build_table(const PackPlan& k, const ConvSpec* const* specs)
{
    PackTable t;
    t.sides = side_forms(k.sets);
    for (const auto& lf : k.layers) add_spec_jobs(t, *specs[lf.first], lf.second);
    return t;
}
// the re-pack of plan k was issued on `packed`: its layers' records become the forms it refreshes (sets = 2 adds them to a forward-only refresh)
static void record_fresh(const void* packed, const PackPlan& k)
{
    std::lock_guard<std::mutex> lk(g_pack_mu);
    PackFresh& r = g_pack_fresh[packed];               // (a buffer never seen starts fully fresh)
    for (const auto& lf : k.layers) r.layer[lf.first] = (k.sets == 2 ? r.layer[lf.first] : 0u) | (lf.second & side_forms(k.sets));
}

struct DevPackTable { PackJob* jobs; PackDgradArgs* dga; int njobs, nblocks; double bytes; std::vector<int> used; };

// one upload per (device, plan); the first call must happen outside stream capture (it allocates)
static const DevPackTable* dev_pack_table(PackPlan k, const ConvSpec* const* specs, int* err)
{
    static std::mutex mu;
    static std::map<PackPlan, DevPackTable> cache;
    if (hipGetDevice(&k.dev) != hipSuccess) { *err = MCVC_ERR_INVALID; return nullptr; }
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(k);
    if (it != cache.end()) return &it->second;
    PackTable t = build_table(k, specs);
    DevPackTable d{};
    d.njobs = (int)t.jobs.size(); d.nblocks = t.nblocks; d.bytes = t.bytes;
    hipError_t e = hipMalloc((void**)&d.jobs, t.jobs.size() * sizeof(PackJob));
    if (e == hipSuccess) e = hipMalloc((void**)&d.dga, t.dga.size() * sizeof(PackDgradArgs));
    if (e == hipSuccess) e = hipMemcpy(d.jobs, t.jobs.data(), t.jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d.dga, t.dga.data(), t.dga.size() * sizeof(PackDgradArgs), hipMemcpyHostToDevice);
    if (e != hipSuccess) { *err = (int)e; return nullptr; }
    for (const PackJob& j : t.jobs) d.used.push_back(j.param);
    return &cache.emplace(std::move(k), std::move(d)).first->second;
}

static int pack_net(const DevPackTable* t, const float* const* params, float* packed, hipStream_t s)
{
    PackPtrs ptrs{};
    for (int i : t->used) { if (i < 0 || i >= 128) return MCVC_ERR_INVALID; ptrs.p[i] = params[i]; }
    return mcvc_pack_net_launch(t->jobs, t->njobs, t->nblocks, t->dga, ptrs, packed, t->bytes, s);
}

// ---- optimizer step fused with the re-pack (pack.h: UpdOwner) -----------------------------------------------------------------------
// The job table of a re-pack (same plan as dev_pack_table) is re-grouped by parameter: every tensor of the parameter range gets ONE owner
// -- a tiled owner whose workgroups update a (CB x IB x taps) block of filters and emit all packed forms of that block, or a flat owner
// (biases, norm affine parameters, tensors nothing is packed from) -- so that one launch is optimizer.step() AND the refresh of every
// copy the kernels read (reference train.py:242,299).
struct DevUpdTable { UpdOwner* owners; PackJob* jobs; PackDgradArgs* dga; int nown, nblocks; double adam_floats, pack_bytes; std::vector<int> used;
                     std::vector<long long> sizes;         // sizes[k]: element count of parameter used[k] the tiles were built for
                     double covered_floats; };             // ... of which in tensors a zero_grads == 2 update leaves uncleared (UpdOwner::covered)

// host half: the owners and the re-ordered jobs (no device call)
struct UpdPlan { std::vector<UpdOwner> owners; std::vector<PackJob> jobs; int nblocks = 0; double adam_floats = 0.0, covered_floats = 0.0;
                 std::vector<int> used; std::vector<long long> sizes; };
// the weight tensors of a plan's layers whose gradient writers can store (grad_store_covered): indexed by parameter
static std::vector<char> covered_params(const PackPlan& k, const ConvSpec* const* specs)
{
    std::vector<char> cov(128, 0);
    for (const auto& lf : k.layers) {
        const ConvSpec& c = *specs[lf.first];
        if (!grad_store_covered(c)) continue;
        for (int br = 0; br < c.nbr; ++br) if (c.wi[br] >= 0 && c.wi[br] < 128) cov[c.wi[br]] = 1;
    }
    return cov;
}
static int plan_upd(const PackTable& t, const long long* numel, int nparams, const std::vector<char>& in_range, const std::vector<char>& covered, UpdPlan& u)
{
    std::vector<PackJob>& jobs = u.jobs;                  // re-ordered: the emits of one parameter are consecutive
    std::vector<UpdOwner>& owners = u.owners;
    int nblocks = 0;
    for (int prm = 0; prm < nparams && prm < 128; ++prm) {
        std::vector<PackJob> mine;
        for (const PackJob& j : t.jobs) if (j.param == prm) mine.push_back(j);
        if (!in_range[prm]) { if (!mine.empty()) return MCVC_ERR_INVALID; continue; }
        if (numel[prm] <= 0) { if (!mine.empty()) return MCVC_ERR_INVALID; continue; }       // (dead parameter)
        UpdOwner o{};
        o.param = prm; o.block0 = nblocks; o.e0 = (int)jobs.size(); o.ne = (int)mine.size();
        bool weight = false;
        for (const PackJob& j : mine) weight = weight || j.kind != PACK_COPY;
        if (!weight) {
            o.flat = 1; o.Cout = (int)numel[prm]; o.Cin = o.taps = 1; o.gx = 1;
            for (const PackJob& j : mine) if (j.Cout != o.Cout) return MCVC_ERR_INVALID;
            nblocks += cdiv_i(o.Cout, 256);
        } else {
            const PackJob& j0 = mine[0];
            o.Cout = j0.Cout; o.Cin = j0.Cin; o.taps = j0.taps;
            for (const PackJob& j : mine) if (j.kind == PACK_COPY || j.Cout != o.Cout || j.Cin != o.Cin || j.taps != o.taps) return MCVC_ERR_INVALID;
            // (the Winograd weight transforms read ONE 5 x 5 filter = 25 consecutive LDS words: upd_emit_filters)
            for (const PackJob& j : mine) if (j.kind >= PACK_WINO_F && j.kind <= PACK_WINO43_F && j.taps != 25) return MCVC_ERR_INVALID;
            if ((long long)o.Cout * o.Cin * o.taps != numel[prm]) return MCVC_ERR_INVALID;
            // tile: 32 x 16 filters of 25 taps (the Winograd layers: two filters per thread), 32 x 32 of 9, 32 x 64 of 3, 32 x 128 of 1;
            // the 5 x 15 edge layers (2 input channels / 1 output channel) as they come
            int cb = 32, ib = 32;
            // (25 taps: 32 x 16 filters = two per thread, 52 KB of LDS -- full 128-byte runs in the forward-type copies; measured against
            //  16 x 16: the family 0.733 -> 0.716 ms per bs=1 iteration, 1.26 -> 1.19 at bs=8.  MCVC_UPD_CB25=16 for the A/B)
            static const int cb25 = mcvc_knob("MCVC_UPD_CB25", 32);
            if (o.taps == 25) { cb = cb25 == 16 ? 16 : 32; ib = 16; }
            else if (o.taps == 3) ib = 64;
            else if (o.taps == 1) ib = 128;
            else if (o.taps > 25) ib = 16;
            o.CB = cb < o.Cout ? cb : o.Cout; o.IB = ib < o.Cin ? ib : o.Cin;
            if ((size_t)o.CB * mcvc_upd_pitch(o.IB, o.taps) * sizeof(float) > kUpdLds) return MCVC_ERR_INVALID;
            o.vec4 = ((o.IB * o.taps) % 4 == 0 && (o.Cin % o.IB) == 0 && ((long long)o.Cin * o.taps) % 4 == 0) ? 1 : 0;
            o.gx = cdiv_i(o.Cin, o.IB);
            nblocks += o.gx * cdiv_i(o.Cout, o.CB);
        }
        o.covered = (!o.flat && covered[prm]) ? 1 : 0;
        u.adam_floats += (double)numel[prm];
        if (o.covered) u.covered_floats += (double)numel[prm];
        for (const PackJob& j : mine) jobs.push_back(j);
        owners.push_back(o);
        u.used.push_back(prm); u.sizes.push_back(numel[prm]);
    }
    if (jobs.size() != t.jobs.size() || owners.empty()) return MCVC_ERR_INVALID;
    u.nblocks = nblocks;
    return 0;
}

static const DevUpdTable* dev_upd_table(PackPlan k, const ConvSpec* const* specs, const long long* numel, int nparams, const std::vector<char>& in_range, int* err)
{
    static std::mutex mu;
    static std::map<PackPlan, DevUpdTable> cache;
    if (hipGetDevice(&k.dev) != hipSuccess) { *err = MCVC_ERR_INVALID; return nullptr; }
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(k);
    if (it != cache.end()) return &it->second;
    PackTable t = build_table(k, specs);
    UpdPlan u;
    if (int e = plan_upd(t, numel, nparams, in_range, covered_params(k, specs), u)) { *err = e; return nullptr; }
    DevUpdTable d{};
    d.adam_floats = u.adam_floats; d.covered_floats = u.covered_floats; d.used = u.used; d.sizes = u.sizes;
    d.nown = (int)u.owners.size(); d.nblocks = u.nblocks;
    d.pack_bytes = t.wbytes;
    if (u.jobs.empty()) u.jobs.push_back(PackJob{});
    if (t.dga.empty()) t.dga.push_back(PackDgradArgs{});
    hipError_t e = hipMalloc((void**)&d.owners, u.owners.size() * sizeof(UpdOwner));
    if (e == hipSuccess) e = hipMalloc((void**)&d.jobs, u.jobs.size() * sizeof(PackJob));
    if (e == hipSuccess) e = hipMalloc((void**)&d.dga, t.dga.size() * sizeof(PackDgradArgs));
    if (e == hipSuccess) e = hipMemcpy(d.owners, u.owners.data(), u.owners.size() * sizeof(UpdOwner), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d.jobs, u.jobs.data(), u.jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d.dga, t.dga.data(), t.dga.size() * sizeof(PackDgradArgs), hipMemcpyHostToDevice);
    if (e != hipSuccess) { *err = (int)e; return nullptr; }
    return &cache.emplace(std::move(k), std::move(d)).first->second;
}

// the optimizer arguments of the fused update: the gradient(s) and the moments live at the same offsets of their flat buffers as the
// parameters do in theirs (engine.py _FlatGroup), so one float offset per buffer locates them from a parameter pointer
struct UpdOpt { const float* flat; const float* grad; const float* grad2; const float* exp_avg; const float* exp_avg_sq;
                float lr, beta1, beta2, eps; int step; float grad_scale; int zero_grads; };

static int update_net(const DevUpdTable* t, const float* const* params, const long long* numel, float* packed, const UpdOpt& o, hipStream_t s)
{
    for (size_t k = 0; k < t->used.size(); ++k) if (numel[t->used[k]] != t->sizes[k]) return MCVC_ERR_INVALID;      // (the table is cached per configuration)
    if (!o.flat || !o.grad || !o.exp_avg || !o.exp_avg_sq || o.step < 1) return MCVC_ERR_INVALID;
    if (o.zero_grads < 0 || o.zero_grads > 2 || (o.zero_grads == 2 && o.grad2)) return MCVC_ERR_INVALID;      // (store mode: one gradient buffer)
    if ((((uintptr_t)o.flat | (uintptr_t)o.grad | (uintptr_t)o.grad2 | (uintptr_t)o.exp_avg | (uintptr_t)o.exp_avg_sq) & 15) != 0) return MCVC_ERR_INVALID;
    PackPtrs ptrs{};
    for (int i : t->used) { if (i < 0 || i >= 128 || !params[i] || (((uintptr_t)params[i]) & 15) != 0) return MCVC_ERR_INVALID; ptrs.p[i] = params[i]; }
    UpdAdam ad{};
    ad.d_g = o.grad - o.flat; ad.d_m = o.exp_avg - o.flat; ad.d_v = o.exp_avg_sq - o.flat;
    ad.has_g2 = o.grad2 ? 1 : 0; ad.d_g2 = o.grad2 ? o.grad2 - o.flat : 0;
    ad.zero = o.zero_grads;
    ad.c = mcvc_adam_coef(o.lr, o.beta1, o.beta2, o.eps, o.step, o.grad_scale);
    // (zero_grads == 2: 28 B per covered parameter -- its gradient is read and left alone -- and 32 B per uncovered one)
    const double bytes = o.zero_grads == 2 ? 28.0 * t->adam_floats + 4.0 * (t->adam_floats - t->covered_floats) + t->pack_bytes
                                           : (28.0 + (o.grad2 ? 4.0 : 0.0) + (o.zero_grads ? (o.grad2 ? 8.0 : 4.0) : 0.0)) * t->adam_floats + t->pack_bytes;
    return mcvc_update_net_launch(t->owners, t->nown, t->nblocks, t->jobs, t->dga, ptrs, packed, ad, bytes, s);
}

// ---- fused small-batch trunk layer (trunk_kernels.hip) ------------------------------------------------
static bool trunk_enabled()
{
    static const int en = mcvc_knob("MCVC_TRUNK", 1);
    return en != 0;
}

// persistent 13-layer forward (trunk_fwd_net_kernel) instead of one fused launch per layer; knob MCVC_TRUNK_NET=0 for A/B runs
static int g_trunk_net = mcvc_knob("MCVC_TRUNK_NET", 1) != 0;
static bool trunk_net_enabled() { return g_trunk_net != 0; }
static bool trunk_bwd_net_enabled() { return g_trunk_net == 1; }          // (2 = forward only)

// conv1d + bias + IN (+GLU | +residual); input / conv_out in trunk layout [C][B][W4]; y plane (b, c) at y.p + b*y.sb + c*y.sc
static bool trunk_fwd(Exec& ex, const ConvSpec& c, const float* const* P, int g0, int be0, int g1, int be1, CTensor x, Tensor conv_out,
                      float* stats, Tensor y, const float* res)
{
    const int B = x.N, W4 = x.W;
    const int mode = (c.nbr == 2) ? TRUNK_IN_GLU : TRUNK_IN;
    if (!trunk_enabled() || c.KH != 1 || !mcvc_trunk_applies(c.Cin, c.KW, c.Cout, B, W4, mode, 1)) return false;
    if (ex.dry) return true;
    TrunkArgs a{};
    a.a0 = P[c.wi[0]]; a.bias0 = P[c.bi[0]]; a.gamma0 = P[g0]; a.beta0 = P[be0];
    if (c.nbr == 2) { a.a1 = P[c.wi[1]]; a.bias1 = P[c.bi[1]]; a.gamma1 = P[g1]; a.beta1 = P[be1]; }
    a.x = x.p; a.x_sc = x.sc; a.x_sb = x.sb;
    a.Cin = c.Cin; a.KW = c.KW; a.K = c.Cin * c.KW; a.M = c.Cout; a.Mtot = c.cout_tot; a.B = B; a.T4 = W4; a.N = B * W4;
    a.conv_out = conv_out.p; a.c_sc = conv_out.sc; a.c_sb = conv_out.sb;
    a.stats = stats; a.y = y.p; a.res = res; a.y_sn = y.sb; a.y_sc = y.sc; a.eps = kInEps; a.mode = mode;
    ex.fail(mcvc_trunk_launch(a, 1, ex.s));
    return true;
}

// largest K split (power-of-two multiples of `start`) the kernel accepts that still keeps the grid below ~512 workgroups
static int trunk_pick_ksplit(int Cin, int KW, int M, int B, int W4, int must_split)
{
    int best = 0;
    for (int ks = 1; ks <= 64; ++ks) {
        if (!mcvc_trunk_applies(Cin, KW, M, B, W4, TRUNK_PLAIN, ks)) continue;
        if (best == 0) best = ks;
        if ((M / 16) * ks <= 512) best = ks;
    }
    (void)must_split;
    return best;
}

// dX[ci][b][t] (+)= sum_{co,kw} W[co][ci][kw] dY[co][b][t + pw - kw]  through the transposed pack.  Large K (or an
// accumulating destination) is split over workgroups that add atomically; a non-accumulating destination is zeroed first.
struct TrunkPre {              // fused InstanceNorm backward in front of the data-gradient (trunk.h)
    int kind;                  // 1 plain IN, 2 IN + gated GLU
    const float* x; const float* stats;
    const float* g0; const float* b0; const float* g1; const float* b1;
    float* out;                // X' = gradient w.r.t. the conv output (the weight gradient reads it)
    float* dg0; float* db0; float* dg1; float* db1;
    int xB;                    // samples per channel of x (0 = the pass's batch; larger: backward over a prefix of the forward pass's samples)
};

static bool trunk_dgrad(Exec& ex, const ConvSpec& c, const float* packed, CTensor dy, Tensor dx, int accumulate,
                        int* nsplit = nullptr, const TrunkPre* pre = nullptr)
{
    const int B = dx.N, W4 = dx.W;
    if (!trunk_enabled() || c.off[PF_TRUNK_T] < 0) return false;
    int ks = 1;
    if (!accumulate && mcvc_trunk_applies(c.cout_tot, c.KW, c.Cin, B, W4, TRUNK_PLAIN, 1)) ks = 1;
    else ks = trunk_pick_ksplit(c.cout_tot, c.KW, c.Cin, B, W4, 0);
    if (ks < 1) return false;
    if (!accumulate && ks > 1 && !nsplit) return false;             // slabs need a consumer that sums them
    const long long tot = (long long)c.Cin * B * W4;
    // deterministic mode: an accumulating K split leaves dx alone and writes ks private slabs; the consumer sums dx + slabs
    const bool slab_all = accumulate && ks > 1 && nsplit && mcvc_deterministic();
    if (ks > 1 && (!accumulate || nsplit)) {
        const long long need = (long long)(accumulate ? ks : ks - 1) * tot;      // (sized for both modes)
        if (need > ex.slab_need) ex.slab_need = need;
        if (!ex.dry && need > ex.slab_cap) { ex.fail(MCVC_ERR_WORKSPACE); return true; }
    }
    if (nsplit) *nsplit = slab_all ? ks + 1 : (accumulate ? 1 : ks);
    if (ex.dry) return true;
    TrunkArgs a{};
    a.a0 = packed + c.off[PF_TRUNK_T];
    a.x = dy.p; a.x_sc = dy.sc; a.x_sb = dy.sb;
    a.Cin = c.cout_tot; a.KW = c.KW; a.K = c.cout_tot * c.KW; a.M = c.Cin; a.Mtot = c.Cin; a.B = B; a.T4 = W4; a.N = B * W4;
    a.conv_out = dx.p; a.c_sc = dx.sc; a.c_sb = dx.sb; a.accumulate = accumulate; a.mode = TRUNK_PLAIN;
    a.slabs = ex.slabs; a.slab_stride = tot; a.slab_all = slab_all ? 1 : 0;
    if (pre) {
        a.pre = pre->kind; a.pre_C = (pre->kind == 2) ? c.cout_tot / 2 : c.cout_tot;
        a.pre_x = pre->x; a.pre_xB = pre->xB; a.pre_stats = pre->stats; a.pre_gamma0 = pre->g0; a.pre_beta0 = pre->b0; a.pre_gamma1 = pre->g1; a.pre_beta1 = pre->b1;
        a.pre_out = pre->out; a.pre_dgamma0 = pre->dg0; a.pre_dbeta0 = pre->db0; a.pre_dgamma1 = pre->dg1; a.pre_dbeta1 = pre->db1;
        wait_readers(ex, pre->out);
    }
    ex.fail(mcvc_trunk_launch(a, ks, ex.s));
    return true;
}

// K too large for one workgroup (conv2dto1d, K = 5120): K-split workgroups write private slabs (split 0 adds the bias) that
// the InstanceNorm launch sums -- no atomics, no zero-fill.  Weights are read straight from the OIHW parameter.
static bool trunk_fwd_ksplit(Exec& ex, const ConvSpec& c, const float* const* P, CTensor x, Tensor conv_out, int* nsplit)
{
    const int B = x.N, W4 = x.W;
    if (!trunk_enabled() || c.KH != 1 || c.nbr != 1) return false;
    const int ks = trunk_pick_ksplit(c.Cin, c.KW, c.Cout, B, W4, 1);
    if (ks < 1) return false;
    const long long tot = (long long)c.Cout * B * W4;
    const long long need = (long long)(ks - 1) * tot;
    if (need > ex.slab_need) ex.slab_need = need;
    if (!ex.dry && need > ex.slab_cap) { ex.fail(MCVC_ERR_WORKSPACE); return true; }
    *nsplit = ks;
    if (ex.dry) return true;
    TrunkArgs a{};
    a.a0 = P[c.wi[0]]; a.bias0 = P[c.bi[0]];
    a.x = x.p; a.x_sc = x.sc; a.x_sb = x.sb;
    a.Cin = c.Cin; a.KW = c.KW; a.K = c.Cin * c.KW; a.M = c.Cout; a.Mtot = c.Cout; a.B = B; a.T4 = W4; a.N = B * W4;
    a.conv_out = conv_out.p; a.c_sc = conv_out.sc; a.c_sb = conv_out.sb; a.accumulate = 0; a.mode = TRUNK_PLAIN;
    a.slabs = ex.slabs; a.slab_stride = tot;
    ex.fail(mcvc_trunk_launch(a, ks, ex.s));
    return true;
}

// ---- norm wrappers -------------------------------------------------------------------------------------
struct NormP { const float* g[2]; const float* b[2]; float* dg[2]; float* db[2]; };

static NormP normp(const float* const* params, float* const* grads, int g0, int b0, int g1 = -1, int b1 = -1)
{
    NormP n{};
    if (!params) return n;                       // dry (sizing) run
    n.g[0] = params[g0]; n.b[0] = params[b0];
    if (g1 >= 0) { n.g[1] = params[g1]; n.b[1] = params[b1]; }
    if (grads) {
        n.dg[0] = grads[g0]; n.db[0] = grads[b0];
        if (g1 >= 0) { n.dg[1] = grads[g1]; n.db[1] = grads[b1]; }
    }
    return n;
}

static int fuse_wino_norm()
{
    static const int en = mcvc_knob("MCVC_FUSE_WINO_NORM", 1);
    return en;
}

// x: the conv output (2C channels in front of a GLU) with its `nslab - 1` K-split slabs; y gives the shape, and its layout the store
// (phase-split padded when y feeds an implicit-GEMM layer)
static void norm_fwd(Exec& ex, Tensor x, int nslab, const NormP& np, float* stats, Tensor y, const float* res, int act)
{
    if (ex.dry) return;
    NormArgs a{};
    a.x = x.p; a.x_slabs = ex.slabs; a.x_sn = x.sb; a.x_sc = x.sc; a.slab_stride = x.dense(); a.nslab = nslab;
    a.gamma[0] = np.g[0]; a.gamma[1] = np.g[1]; a.beta[0] = np.b[0]; a.beta[1] = np.b[1];
    a.stats = stats; a.y = y.p; a.res = res; a.y_sn = y.sb; a.y_sc = y.sc; a.y_sh = y.sh;
    a.N = y.N; a.C = y.C; a.H = y.H; a.W = y.W; a.act = act; a.eps = kInEps;
    if (y.lay == L_PHASE_SPLIT) { a.y_xs = 1; a.xs_pw = mcvc_xs_pw(y.W); a.xs_plane = mcvc_xs_plane(y.H, y.W); }
    if (ex.pend_fam) {
        const WinoFam& f = *ex.pend_fam;
        ex.pend_fam = nullptr;
        if (mcvc_norm_fwd_wino_applies(a, ex.pend, f.norm_pts)) { ex.fail(mcvc_norm_fwd_wino_launch(a, ex.pend, f.norm_pts, ex.s)); return; }
        ex.fail(f.output(ex.pend, ex.s));
    }
    ex.fail(mcvc_norm_fwd_launch(a, ex.s));
}

// dy: the gradient of the norm's output with its slabs, it gives the shape; dx: the conv output's gradient -- un-shuffled into conv-output
// coordinates behind a PixelShuffle (`unshuffle`), in the padded dY layout when an implicit data gradient reads it
static void norm_bwd(Exec& ex, CTensor x, const NormP& np, const float* stats, Tensor dy, int nslab, Tensor dx, int unshuffle, int act)
{
    if (ex.dry) return;
    wait_readers(ex, dx.p);
    NormBwdArgs a{};
    a.x = x.p; a.x_sn = x.sb; a.x_sc = x.sc;
    a.gamma[0] = np.g[0]; a.gamma[1] = np.g[1]; a.beta[0] = np.b[0]; a.beta[1] = np.b[1];
    a.stats = stats; a.dy = dy.p; a.dy_slabs = ex.slabs; a.y_sn = dy.sb; a.y_sc = dy.sc; a.y_sh = dy.sh; a.slab_stride = dy.dense(); a.nslab = nslab;
    a.dx = dx.p; a.dx_sn = dx.sb; a.dx_sc = dx.sc; a.dx_sh = dx.sh; a.unshuffle = unshuffle;
    a.dgamma[0] = np.dg[0]; a.dgamma[1] = np.dg[1]; a.dbeta[0] = np.db[0]; a.dbeta[1] = np.db[1];
    a.N = dy.N; a.C = dy.C; a.H = dy.H; a.W = dy.W; a.act = act;
    a.dx_pitch = dx.lay == L_PADDED_DY ? dx.sh : 0;
    ex.fail(mcvc_norm_bwd_launch(a, ex.s));
}

// dense tensors; y gives the shape (x has 2C channels in front of a GLU)
static void act_fwd(Exec& ex, Tensor x, int nslab, Tensor y, int act)
{
    if (ex.dry) return;
    ActArgs a{}; a.x = x.p; a.x_slabs = ex.slabs; a.slab_stride = x.dense(); a.nslab = nslab; a.y = y.p; a.N = y.N; a.C = y.C; a.P = y.P(); a.act = act;
    ex.fail(mcvc_act_fwd_launch(a, ex.s));
}
// the K-split slabs of t added into it, in place
static void sum_slabs(Exec& ex, Tensor t, int nslab)
{
    if (nslab > 1) act_fwd(ex, t, nslab, t.at(nullptr), ACT_NONE);
}

static void act_bwd(Exec& ex, CTensor x, Tensor dy, int nslab, Tensor dx, int act)
{
    if (ex.dry) return;
    wait_readers(ex, dx.p);
    ActBwdArgs a{}; a.x = x.p; a.dy = dy.p; a.dy_slabs = ex.slabs; a.slab_stride = dy.dense(); a.nslab = nslab; a.dx = dx.p; a.N = dy.N; a.C = dy.C; a.P = dy.P(); a.act = act;
    ex.fail(mcvc_act_bwd_launch(a, ex.s));
}

// ---- stash: one table per network ---------------------------------------------------------------------------------------------------------
// SK_BATCH: dense, batch-major.  SK_TRUNK: the 1-D trunk's [C][stash_B][W].  SK_STATS: 2 floats per channel and sample.  SK_SPLIT: the input
// of a 3x3 stride-2 layer -- phase-split padded when the pass runs those layers as implicit GEMMs, dense otherwise; sized for the larger form.
enum StashKind { SK_BATCH, SK_TRUNK, SK_STATS, SK_SPLIT };
struct StashRow { int C, H, W; StashKind kind; };
constexpr int kMaxStashRows = 64;
struct Stash {
    int n;
    long long off[kMaxStashRows], floats[kMaxStashRows], win[kMaxStashRows], total;      // win: offset of the pass's first sample
    Tensor t[kMaxStashRows];                               // as the pass addresses them: from its first sample on
    const Tensor& operator[](int i) const { return t[i]; }
};
// Rows laid out back to back (each rounded up to 4 floats) for stash_B samples; the tensors are those of a pass over B samples from sample b0
// on: a window moves every tensor by b0 x its sample stride -- a sample's floats when batch-major, W when the batch sits inside the channel.
static Stash stash_layout(const StashRow* rows, int n, float* base, int B, int stash_B, int b0, bool split)
{
    Stash s{};
    s.n = n;
    for (int i = 0; i < n; ++i) {
        const StashRow& r = rows[i];
        long long per = (long long)r.C * r.H * r.W;       // floats per sample
        Tensor t{};
        switch (r.kind) {
        case SK_BATCH: t = nchw(base, B, r.C, r.H, r.W); break;
        case SK_TRUNK: t = trunk_rows(base, B, r.C, r.W, (long long)stash_B * r.W); break;
        case SK_STATS: t = nchw(base, B, r.C, 1, 2); per = 2LL * r.C; break;
        case SK_SPLIT: {
            const long long xs = (r.H & 1) || (r.W & 1) ? 0 : mcvc_xs_floats(r.C, r.H, r.W);
            t = split ? phase_split(base, B, r.C, r.H, r.W) : nchw(base, B, r.C, r.H, r.W);
            if (xs > per) per = xs;
        } break;
        }
        s.off[i] = s.total; s.floats[i] = stash_B * per;
        s.win[i] = s.total + b0 * t.sb;
        t.p += s.win[i];
        s.t[i] = t;
        s.total += (s.floats[i] + 3) & ~3LL;
    }
    return s;
}

// =================================================================================================
// Generator
// =================================================================================================
struct GenNet {
    ConvSpec conv1, ds1, ds2, c2d1d, res_vg[6], res_out[6], c1d2d, up1, up2, last;
    long long packed_floats;
};

// the layers in ConvSpec::index order = their order in the packed buffer
static void gen_layers(const GenNet& g, const ConvSpec** l)
{
    const ConvSpec* head[] = {&g.conv1, &g.ds1, &g.ds2, &g.c2d1d, &g.c1d2d, &g.up1, &g.up2, &g.last};
    for (int i = 0; i < 8; ++i) l[i] = head[i];
    for (int i = 0; i < 6; ++i) { l[8 + 2 * i] = &g.res_vg[i]; l[9 + 2 * i] = &g.res_out[i]; }
}
static GenNet build_gen()
{
    GenNet g{};
    long long cur = 0;
    g.conv1 = mk(2, 128, 2, 5, 15, 1, 2, 7, 0, 1, 2, 3, 1);            // model.py:116-126 (no norm -> bias grads live)
    g.ds1 = mk(128, 256, 2, 5, 5, 2, 2, 2, 4, 5, 8, 9, 0);              // :129-133
    g.ds2 = mk(256, 256, 2, 5, 5, 2, 2, 2, 12, 13, 16, 17, 0);          // :135-139
    g.c2d1d = mk(5120, 256, 1, 1, 1, 1, 0, 0, 20, 21, -1, -1, 0);       // :142-146
    for (int i = 0; i < 6; ++i) {                                       // :151-180
        const int b = 24 + 12 * i;
        g.res_vg[i] = mk(256, 512, 2, 1, 3, 1, 0, 1, b + 0, b + 1, b + 4, b + 5, 0);
        g.res_out[i] = mk(512, 256, 1, 1, 3, 1, 0, 1, b + 8, b + 9, -1, -1, 0);
    }
    g.c1d2d = mk(256, 5120, 1, 1, 1, 1, 0, 0, 96, 97, -1, -1, 0);       // :183-187
    g.up1 = mk(256, 1024, 1, 5, 5, 1, 2, 2, 104, 105, -1, -1, 1);       // :192-196 (PixelShuffle before the norm -> bias grad live)
    g.up2 = mk(256, 512, 1, 5, 5, 1, 2, 2, 100, 101, -1, -1, 1);        // :200-204 (named convLayer.* in named_parameters)
    g.last = mk(128, 1, 1, 5, 15, 1, 2, 7, 108, 109, -1, -1, 1);        // :207-211
    const ConvSpec* l[kMaxLayers];
    gen_layers(g, l);
    for (int i = 0; i < kMaxLayers; ++i) { ConvSpec& c = const_cast<ConvSpec&>(*l[i]); c.index = i; spec_finalize(c, cur); }      // (g itself is not const)
    g.packed_floats = cur;
    return g;
}
static const GenNet& gen_net() { static const GenNet g = build_gen(); return g; }
static const ConvSpec* const* gen_specs()
{
    static const ConvSpec* l[kMaxLayers];
    static const bool once = (gen_layers(gen_net(), l), true);
    (void)once;
    return l;
}

struct GenDims {
    int B, T, W2, W4, Wu1, Wu2;
    long long big;       // largest activation / conv-output tensor (floats)
};
static GenDims gen_dims(int B, int T)
{
    GenDims d{};
    d.B = B; d.T = T;
    d.W2 = conv_out(T, 5, 2, 2);
    d.W4 = conv_out(d.W2, 5, 2, 2);
    d.Wu1 = 2 * d.W4; d.Wu2 = 4 * d.W4;
    const int wmax = d.T > d.Wu2 ? d.T : d.Wu2;
    d.big = (long long)B * 256 * 80 * wmax;
    return d;
}

// What the forward pass leaves for the backward pass, one row per tensor in stash order: c* conv outputs (a norm's input, value | gate
// channels in front of a GLU), s* the norm's statistics, y* the layer outputs.  Offsets, window shifts and the walks' tensors all come
// from here (stash_layout).
enum { WT, WW2, WW4, WWU1, WWU2 };                         // which of GenDims' widths a row has
enum GenStashId { GS_XIN, GS_C1, GS_Y1, GS_C2, GS_S2, GS_Y2, GS_C3, GS_S3, GS_Y3, GS_C4, GS_S4, GS_Y4,
                  GS_RES,                                  // six residual blocks of six rows: GS_RES + 6 * i + R_*
                  GS_C6 = GS_RES + 36, GS_S6, GS_Y6, GS_C7, GS_S7, GS_Y7, GS_C8, GS_S8, GS_Y8, GS_ROWS };
enum { R_CA, R_SA, R_YA, R_CB, R_SB, R_Y };
struct GenStashRow { int C, H, width; StashKind kind; };
static const GenStashRow kGenStashHead[] = {
    {2, 80, WT, SK_BATCH},                                                                           // stack(x * mask, mask)
    {256, 80, WT, SK_BATCH}, {128, 80, WT, SK_BATCH},                                                // conv1 | GLU
    {512, 40, WW2, SK_BATCH}, {512, 1, 0, SK_STATS}, {256, 40, WW2, SK_BATCH},                       // downSample1
    {512, 20, WW4, SK_BATCH}, {512, 1, 0, SK_STATS}, {5120, 1, WW4, SK_TRUNK},                       // downSample2, stored [c*20+h][b][w]
    {256, 1, WW4, SK_TRUNK}, {256, 1, 0, SK_STATS}, {256, 1, WW4, SK_TRUNK}};                        // conv2dto1d
static const GenStashRow kGenStashBlock[] = {
    {1024, 1, WW4, SK_TRUNK}, {1024, 1, 0, SK_STATS}, {512, 1, WW4, SK_TRUNK},                       // value | gate convs, GLU
    {256, 1, WW4, SK_TRUNK}, {256, 1, 0, SK_STATS}, {256, 1, WW4, SK_TRUNK}};                        // out conv + skip
static const GenStashRow kGenStashTail[] = {
    {5120, 1, WW4, SK_TRUNK}, {5120, 1, 0, SK_STATS}, {256, 20, WW4, SK_BATCH},                      // conv1dto2d, stored NCHW
    {256, 40, WWU1, SK_BATCH}, {256, 1, 0, SK_STATS}, {256, 40, WWU1, SK_BATCH},                     // upSample1 (behind its PixelShuffle)
    {128, 80, WWU2, SK_BATCH}, {128, 1, 0, SK_STATS}, {128, 80, WWU2, SK_BATCH}};                    // upSample2
// the generator's stash written by a pass over stash_B samples of d.T frames, as a pass over d.B samples from sample b0 on addresses it
static Stash gen_stash(float* base, const GenDims& d, int stash_B, int b0 = 0)
{
    const int widths[] = {d.T, d.W2, d.W4, d.Wu1, d.Wu2};
    StashRow rows[GS_ROWS];
    int n = 0;
    auto add = [&](const GenStashRow* r, int k) { for (; k > 0; --k, ++r) rows[n++] = StashRow{r->C, r->H, widths[r->width], r->kind}; };
    add(kGenStashHead, GS_RES);
    for (int i = 0; i < 6; ++i) add(kGenStashBlock, 6);
    add(kGenStashTail, GS_ROWS - GS_C6);
    return stash_layout(rows, GS_ROWS, base, d.B, stash_B, b0, false);
}

struct GenScratch {
    long long ga, gb, gb2, dh, dt1, dt1b, dt2, dt3, dt3b, dtx1, dtx3, wv, wm, wino_floats, wv2, wm2, wu, wu_floats, sync, slabs;
    int B, W4;
    // a gradient buffer of the 1-D trunk: [C][B][W4], the pass's own batch inside
    Tensor trunk(float* sc, long long off, int C) const { return trunk_rows(sc + off, B, C, W4, (long long)B * W4); }
};
static GenScratch gen_scratch(const GenDims& d)
{
    GenScratch s{};
    s.B = d.B; s.W4 = d.W4;
    long long cur = 0;
    auto take = [&](long long n) { const long long o = cur; cur += (n + 3) & ~3LL; return o; };
    // first, so that its place does not depend on the batch size: callers share one scratch buffer between passes of different batch
    // (the trainer's B and 2B passes), and the sticky error word (mcvc_gen_trunk_fault) must not land inside another layout's data
    s.sync = take(2 * MCVC_TRUNK_SYNC_WORDS);            // forward | backward persistent trunk kernels
    s.ga = take(d.big); s.gb = take(d.big); s.gb2 = take(d.big);
    s.dh = take((long long)256 * d.B * d.W4); s.dt1 = take((long long)1024 * d.B * d.W4); s.dt1b = take((long long)1024 * d.B * d.W4);
    s.dt2 = take((long long)512 * d.B * d.W4); s.dt3 = take((long long)256 * d.B * d.W4); s.dt3b = take((long long)256 * d.B * d.W4);
    // small batch: one conv-output gradient buffer per residual layer, so that ONE batched launch computes all their weight gradients
    s.dtx1 = take(mcvc_wgrad_smallk_batch_applies(d.B, d.W4) ? 6LL * 1024 * d.B * d.W4 : 0);
    s.dtx3 = take(mcvc_wgrad_smallk_batch_applies(d.B, d.W4) ? 6LL * 256 * d.B * d.W4 : 0);
    // Winograd V / M of upSample1 (1024 ch, tiles of a 20 x W4 image) and upSample2 (512 ch, 40 x 2*W4)
    {
        // (a batch beyond kWinoMaxTiles tiles runs in chunks of samples: the workspaces are sized for one chunk)
        const long long nt1 = wino_chunk_tiles(d.B, 10LL * ((d.W4 + 1) / 2)), nt2 = wino_chunk_tiles(d.B, 20LL * ((d.Wu1 + 1) / 2));
        const long long a1 = 36LL * 1024 * nt1, a2 = 36LL * 512 * nt2;
        s.wino_floats = wino_enabled() ? (a1 > a2 ? a1 : a2) : 0;
        s.wv = take(s.wino_floats); s.wm = take(s.wino_floats);
        s.wv2 = take(s.wino_floats); s.wm2 = take(s.wino_floats);
        s.wu_floats = wino_enabled() ? 36LL * 1024 * 1024 : 0;        // dU of downSample2 in phase form, 36 points of F(4x4,3x3) (> upSample1's 64 x 1024 x 256)
        s.wu = take(s.wu_floats);
    }
    s.slabs = cur;
    return s;
}

static void gen_forward_impl(Exec& ex, const float* const* P, const float* packed, const float* x, const float* mask, float* out,
                             float* st, const GenDims& d)
{
    ex.params = P;
    const GenNet& g = gen_net();
    const Stash o = gen_stash(st, d, d.B);
    auto res = [&](int i, int k) -> const Tensor& { return o[GS_RES + 6 * i + k]; };
    const int B = d.B, T = d.T;
    int ns = 1;
    // ---- model.py:241-242  stack(x*mask, mask) -> gated 5x15 conv (value|gate in one launch)
    if (!ex.dry) ex.fail(mcvc_prep_input_launch(x, mask, o[GS_XIN].p, B, 80 * T, ex.s));
    conv_fwd(ex, g.conv1, packed, o[GS_XIN], o[GS_C1], 0, 1, &ns);
    act_fwd(ex, o[GS_C1], ns, o[GS_Y1], ACT_GLU);
    // a 2-D layer: conv (c = its output in the stash; PixelShuffle fused into the store) -> IN -> activation; the norm may absorb a Winograd output transform
    auto conv_norm = [&](const ConvSpec& cs, const Tensor& xin, int c, int shuffle, const NormP& np, const Tensor& y, int act) {
        ex.fuse_next = fuse_wino_norm();
        conv_fwd(ex, cs, packed, xin, o[c], shuffle, 1, &ns);
        ex.fuse_next = 0;
        norm_fwd(ex, o[c], ns, np, o[c + 1].p, y, nullptr, act);
    };
    // ---- :245  downSample1 (5x5 s2, IN, GLU)
    conv_norm(g.ds1, o[GS_Y1], GS_C2, 0, normp(P, nullptr, 6, 7, 10, 11), o[GS_Y2], ACT_GLU);
    // ---- :246  downSample2; output written straight in trunk layout [c*20+h][b][w]  (:249-251)
    conv_norm(g.ds2, o[GS_Y2], GS_C3, 0, normp(P, nullptr, 14, 15, 18, 19), o[GS_Y3].rows20(), ACT_GLU);
    // ---- :254-255  1x1 5120->256 + IN ; image = [5120][B rows][W4]
    if (trunk_fwd_ksplit(ex, g.c2d1d, P, o[GS_Y3], o[GS_C4], &ns)) {}
    else conv_fwd(ex, g.c2d1d, packed, o[GS_Y3].image(), o[GS_C4].image(), 0, 1, &ns);
    norm_fwd(ex, o[GS_C4], ns, normp(P, nullptr, 22, 23), o[GS_S4].p, o[GS_Y4], nullptr, ACT_NONE);
    // ---- :258-271  six residual GLU blocks + 1x1 256->5120 + IN (written as NCHW [B][256][20][W4], 5120 = c*20 + h)
    // a 1-D layer (stash rows c, c + 1: conv output, statistics): the fused kernel where it applies, else a conv over the image of B rows + the norm
    auto layer1d = [&](const ConvSpec& cs, int g0, int be0, int g1, int be1, const Tensor& xin, int c, const Tensor& y, const float* skip, int act) {
        if (trunk_fwd(ex, cs, P, g0, be0, g1, be1, xin, o[c], o[c + 1].p, y, skip)) return;
        conv_fwd(ex, cs, packed, xin.image(), o[c].image(), 0, 1, &ns);
        norm_fwd(ex, o[c], ns, normp(P, nullptr, g0, be0, g1, be1), o[c + 1].p, y, skip, act);
    };
    const Tensor* h = &o[GS_Y4];
    const Tensor y6 = o[GS_Y6].rows_as_channels();
    // small batch: the 12 dependent residual layers in ONE persistent launch (trunk.h)
    const bool persistent = trunk_net_enabled() && trunk_enabled() && ex.sync && mcvc_trunk_net_applies(B, d.W4);
    if (persistent && !ex.dry) {
        TrunkFwdNetArgs na{};
        int l = 0;
        auto fill = [&](const ConvSpec& c, int g0, int be0, int g1, int be1, const Tensor& x, const Tensor* r, const float* skip, int rows) {
            TrunkLayerDesc& d = na.L[l++];           // r: the layer's conv output, statistics and output rows of the stash
            d.a0 = P[c.wi[0]]; d.bias0 = P[c.bi[0]]; d.gamma0 = P[g0]; d.beta0 = P[be0];
            if (c.nbr == 2) { d.a1 = P[c.wi[1]]; d.bias1 = P[c.bi[1]]; d.gamma1 = P[g1]; d.beta1 = P[be1]; }
            d.x = x.p; d.conv_out = r[0].p; d.stats = r[1].p; d.y = r[2].p; d.y_sn = r[2].sb; d.y_sc = r[2].sc; d.res = skip;
            d.Cin = c.Cin; d.KW = c.KW; d.M = c.Cout; d.mode = (c.nbr == 2) ? TRUNK_IN_GLU : TRUNK_IN; d.rows = rows;
        };
        for (int i = 0; i < 6; ++i) {
            const int b = 24 + 12 * i;
            fill(g.res_vg[i], b + 2, b + 3, b + 6, b + 7, *h, &res(i, R_CA), nullptr, 8);
            fill(g.res_out[i], b + 10, b + 11, -1, -1, res(i, R_YA), &res(i, R_CB), h->p, 4);
            h = &res(i, R_Y);
        }
        na.nlayers = l; na.B = B; na.T4 = d.W4; na.eps = kInEps; na.sync = ex.sync;
        ex.fail(mcvc_trunk_fwd_net_launch(na, ex.s));
    }
    for (int i = 0; i < 6 && !persistent; ++i) {
        const int b = 24 + 12 * i;
        layer1d(g.res_vg[i], b + 2, b + 3, b + 6, b + 7, *h, GS_RES + 6 * i + R_CA, res(i, R_YA), nullptr, ACT_GLU);
        layer1d(g.res_out[i], b + 10, b + 11, -1, -1, res(i, R_YA), GS_RES + 6 * i + R_CB, res(i, R_Y), h->p, ACT_NONE);
        h = &res(i, R_Y);
    }
    h = &res(5, R_Y);
    // 1x1 256 -> 5120 + IN: 320 independent row tiles -- its own (wide) launch behind the persistent one, which needs the fused kernel
    if (!persistent) layer1d(g.c1d2d, 98, 99, -1, -1, *h, GS_C6, y6, nullptr, ACT_NONE);
    else if (!trunk_fwd(ex, g.c1d2d, P, 98, 99, -1, -1, *h, o[GS_C6], o[GS_S6].p, y6, nullptr)) ex.fail(MCVC_ERR_INVALID);
    // ---- :274  upSample1: conv 5x5 -> PixelShuffle(2) (fused into the store) -> IN -> x*sigmoid(x)
    conv_norm(g.up1, o[GS_Y6], GS_C7, 1, normp(P, nullptr, 106, 107), o[GS_Y7], ACT_SILU);
    // ---- :275  upSample2
    conv_norm(g.up2, o[GS_Y7], GS_C8, 1, normp(P, nullptr, 102, 103), o[GS_Y8], ACT_SILU);
    // ---- :278-279  last 5x15 conv to one channel
    const Tensor yo = nchw(out, B, 1, 80, d.Wu2);
    conv_fwd(ex, g.last, packed, o[GS_Y8], yo, 0, 1, &ns);
    sum_slabs(ex, yo, ns);
}

// every gradient kernel launched so far (main stream: norm / bias gradients; aux stream: weight gradients) is ordered
// before `ev`
static void record_milestone(Exec& ex, void* ev)
{
    if (!ev || ex.dry) return;
    ex.fail(mcvc_event_record((hipEvent_t)ev, fork_aux(ex)));
}

// `stash_B` > B: the stash was written by a forward pass over stash_B samples and this pass back-propagates through its samples
// [stash_b0, stash_b0 + B) only (the trainer's merged forwards: train.py:203-210 of iteration t+1 batched with :259-273 of iteration t, which
// need no gradient; and the identity sample's backward, which depends on nothing but its own forward, ahead of the others').  The stash
// table hands out the window's tensors (gen_stash): the batch-major ones start b0 samples in, the 1-D trunk's b0 rows in with the stash's
// channel pitch stash_B * W4; the gradients of the trunk (GenScratch::trunk) have the pass's own, B * W4.
static void gen_backward_impl(Exec& ex, const float* const* P, const float* packed, float* const* G, const float* mask, const float* dout,
                              float* dx, int accumulate_dx, const float* stc, float* sc, const GenDims& d, void* const* milestones = nullptr,
                              int stash_B = 0, int stash_b0 = 0)
{
    ex.params = P;
    const GenNet& g = gen_net();
    if (stash_B < d.B) stash_B = d.B;
    // (stash is read-only here; kernels take non-const for slab-reduce paths that are not used on it)
    const Stash o = gen_stash(const_cast<float*>(stc), d, stash_B, stash_b0);
    auto res = [&](int i, int k) -> const Tensor& { return o[GS_RES + 6 * i + k]; };
    const GenScratch q = gen_scratch(d);
    const int B = d.B, T = d.T, W4 = d.W4, Wu1 = d.Wu1, Wu2 = d.Wu2;
    const int pxB = stash_B > B ? stash_B : 0;
    // (float4 paths of the trunk kernels need 16-byte aligned rows: a window that starts at an odd multiple of W4 < 4 floats would not be)
    if (stash_b0 > 0 && (((long long)stash_b0 * W4) & 3)) { ex.fail(MCVC_ERR_INVALID); return; }
    // dY buffers alternate between two copies so an aux-stream weight gradient can still read layer k's dY while the
    // main stream already produces layer k-1's
    float* GA = sc + q.ga;
    float* GBs[2] = {sc + q.gb, sc + q.gb2};
    const Tensor DT1s[2] = {q.trunk(sc, q.dt1, 1024), q.trunk(sc, q.dt1b, 1024)};
    const Tensor DT3s[2] = {q.trunk(sc, q.dt3, 256), q.trunk(sc, q.dt3b, 256)};
    const Tensor DTX1 = q.trunk(sc, q.dtx1, 6 * 1024), DTX3 = q.trunk(sc, q.dtx3, 6 * 256);      // (small batch: a sixth per residual block)
    int gbi = 0;
    auto nextGB = [&]() { gbi ^= 1; return GBs[gbi]; };
    float* GB = GBs[0];
    const Tensor DH = q.trunk(sc, q.dh, 256), DT2 = q.trunk(sc, q.dt2, 512);
    int ns = 1;
    // one 2-D layer behind its norm: weight, bias and data gradient of conv c from dY (conv-output layout) and the stashed input x
    auto conv_bwd = [&](const ConvSpec& c, CTensor x, CTensor dy, Tensor dx_) {
        conv_wgrad(ex, c, G, x, dy);
        conv_bias_grad(ex, c, G, dy);
        conv_dgrad(ex, c, packed, dy, dx_, 0, 1, &ns);
    };
    // ---- last conv (model.py:278)
    conv_bwd(g.last, o[GS_Y8], nchw(dout, B, 1, 80, Wu2), o[GS_Y8].at(GA));
    // ---- upSample2 (:275): IN+SiLU backward, un-shuffled into conv-output coordinates [B][512][40][Wu1]
    GB = nextGB();
    norm_bwd(ex, o[GS_C8], normp(P, G, 102, 103), o[GS_S8].p, o[GS_C8].at(GA), ns, nchw(GB, B, 512, 40, Wu1), 1, ACT_SILU);
    conv_bwd(g.up2, o[GS_Y7], nchw(GB, B, 512, 40, Wu1), o[GS_Y7].at(GA));
    // ---- upSample1 (:274)
    GB = nextGB();
    norm_bwd(ex, o[GS_C7], normp(P, G, 106, 107), o[GS_S7].p, o[GS_C7].at(GA), ns, nchw(GB, B, 1024, 20, W4), 1, ACT_SILU);
    conv_bwd(g.up1, o[GS_Y6], nchw(GB, B, 1024, 20, W4), o[GS_Y6].at(GA));
    if (milestones) record_milestone(ex, milestones[0]);          // parameters [100,110) are done
    // ---- conv1dto2d + IN (:266-271): dy arrives NCHW, dx leaves in trunk layout
    GB = nextGB();
    const Tensor dy6 = q.trunk(GB, 0, 5120);
    norm_bwd(ex, o[GS_C6], normp(P, G, 98, 99), o[GS_S6].p, o[GS_Y6].at(GA).rows_as_channels(), ns, dy6, 0, ACT_NONE);
    conv_wgrad(ex, g.c1d2d, G, res(5, R_Y).image(), dy6.image());
    if (trunk_dgrad(ex, g.c1d2d, packed, dy6, DH, 0, &ns)) {}
    else conv_dgrad(ex, g.c1d2d, packed, dy6.image(), DH.image(), 0, 1, &ns);
    // ---- residual blocks (:258-263), last to first.  DH carries d(h) and is updated in place.
    // small batch: the InstanceNorm backward of each layer is recomputed inside the data-gradient launch that consumes it (one thread
    // per channel of the workgroup's K slice) -- 2 dependent launches per residual block instead of 4.  Needs an un-split upstream
    // gradient (the fused staging does not sum slabs) and the fused data-gradient kernels for both convs of the block.
    static const int fuse_knob = mcvc_knob("MCVC_TRUNK_BWD_FUSE", 1);
    static const int batch_knob = mcvc_knob("MCVC_TRUNK_WGRAD_BATCH", 1);
    SmallKJob wjobs[MCVC_SMALLK_MAX_JOBS];
    int nwjobs = 0;
    const bool batch_w = batch_knob && mcvc_wgrad_smallk_batch_applies(B, W4) && (W4 <= 128);
    auto wstore = [&](const ConvSpec& c) { return (ex.store_grads && grad_store_covered(c)) ? 1 : 0; };      // (the batched launch's per-job flag)
    // the weight gradients of block i, queued for the batched launch behind the chain: out conv, value conv, gate conv
    auto queue_wgrads = [&](int i, const Tensor& hin, const Tensor& dt3, const Tensor& dt1) {
        wjobs[nwjobs++] = SmallKJob{res(i, R_YA).p, dt3.p, G[g.res_out[i].wi[0]], 512, 256, pxB, wstore(g.res_out[i])};
        wjobs[nwjobs++] = SmallKJob{hin.p, dt1.p, G[g.res_vg[i].wi[0]], 256, 512, pxB, wstore(g.res_vg[i])};
        wjobs[nwjobs++] = SmallKJob{hin.p, dt1.channels(512, 512).p, G[g.res_vg[i].wi[1]], 256, 512, pxB, wstore(g.res_vg[i])};
    };
    // Persistent backward (trunk.h): the 12 dependent data-gradient layers of the six blocks in ONE launch, when every layer would take the
    // fused path anyway, the gradient arriving from conv1dto2d is not split into slabs and the staged gradients fit the LDS
    static const int bwd_net_knob = mcvc_knob("MCVC_TRUNK_BWD_NET", 1);
    bool bwd_net = bwd_net_knob && trunk_bwd_net_enabled() && fuse_knob && trunk_enabled() && batch_w && !ex.dry && G && ex.sync &&
                   mcvc_trunk_bwd_net_applies(B, W4);
    for (int i = 0; i < 6 && bwd_net; ++i)
        bwd_net = g.res_out[i].off[PF_TRUNK_T] >= 0 && g.res_vg[i].off[PF_TRUNK_T] >= 0 && mcvc_trunk_applies(g.res_out[i].cout_tot, 3, g.res_out[i].Cin, B, W4, TRUNK_PLAIN, 1);
    if (bwd_net) {
        TrunkBwdNetArgs na{};
        int l = 0;
        for (int i = 5; i >= 0; --i) {
            const int b = 24 + 12 * i;
            const Tensor& hin = (i == 0) ? o[GS_Y4] : res(i - 1, R_Y);
            const Tensor dt3 = DTX3.channels(i * 256, 256), dt1 = DTX1.channels(i * 1024, 1024);
            TrunkBwdLayerDesc& da = na.L[l++];           // conv1d_out_layer (512 -> 256) + its InstanceNorm: d(h_out) -> d(GLU output)
            da.wt = packed + g.res_out[i].off[PF_TRUNK_T]; da.dy = DH.p; da.px = res(i, R_CB).p; da.stats = res(i, R_SB).p;
            da.g0 = P[b + 10]; da.b0 = P[b + 11]; da.xout = dt3.p; da.pxB = pxB; da.dg0 = G[b + 10]; da.db0 = G[b + 11];
            da.out = DT2.p; da.pre = 1; da.C = 256; da.M = 512; da.rows = 8;
            da.flags = (i < 5 ? TBWD_DY_FRESH : 0) | ((i == 5 && ns > 1) ? TBWD_SLAB_DY : 0);            // (conv1dto2d's K-split slabs)
            TrunkBwdLayerDesc& db = na.L[l++];           // value | gate convs (256 -> 512 each) + norms + GLU: d(GLU output) -> d(h_in), added to the skip path
            db.wt = packed + g.res_vg[i].off[PF_TRUNK_T]; db.dy = DT2.p; db.px = res(i, R_CA).p; db.stats = res(i, R_SA).p;
            db.g0 = P[b + 2]; db.b0 = P[b + 3]; db.g1 = P[b + 6]; db.b1 = P[b + 7]; db.xout = dt1.p; db.pxB = pxB;
            db.dg0 = G[b + 2]; db.db0 = G[b + 3]; db.dg1 = G[b + 6]; db.db1 = G[b + 7];
            db.out = DH.p; db.pre = 2; db.C = 512; db.M = 256; db.rows = 4;
            db.flags = TBWD_ACCUMULATE | TBWD_DY_FRESH | ((i == 5 && ns > 1) ? TBWD_SLAB_OUT : 0);
            queue_wgrads(i, hin, dt3, dt1);
        }
        na.nlayers = l; na.B = B; na.T4 = W4; na.slabs = ex.slabs; na.slab_stride = DH.dense(); na.nslab = ns; na.sync = ex.sync + MCVC_TRUNK_SYNC_WORDS; na.err = ex.sync + MCVC_TRUNK_SYNC_WORDS - 1;
        for (int i = 0; i < 6; ++i) { wait_readers(ex, DTX3.channels(i * 256, 256).p); wait_readers(ex, DTX1.channels(i * 1024, 1024).p); }
        ex.fail(mcvc_trunk_bwd_net_launch(na, ex.s));
        ns = 1;
    }
    for (int i = 5; i >= 0 && !bwd_net; --i) {
        const int b = 24 + 12 * i;
        const Tensor& hin = (i == 0) ? o[GS_Y4] : res(i - 1, R_Y);
        Tensor DT3 = DT3s[i & 1], DT1 = DT1s[i & 1];
        const bool fuse = fuse_knob && trunk_enabled() && ns == 1 && !ex.dry && G && g.res_out[i].off[PF_TRUNK_T] >= 0 && g.res_vg[i].off[PF_TRUNK_T] >= 0 &&
                          mcvc_trunk_applies(g.res_out[i].cout_tot, 3, g.res_out[i].Cin, B, W4, TRUNK_PLAIN, 1) &&
                          trunk_pick_ksplit(g.res_vg[i].cout_tot, 3, g.res_vg[i].Cin, B, W4, 0) >= 1;
        if (fuse) {
            if (batch_w) { DT3 = DTX3.channels(i * 256, 256); DT1 = DTX1.channels(i * 1024, 1024); }
            TrunkPre pa{1, res(i, R_CB).p, res(i, R_SB).p, P[b + 10], P[b + 11], nullptr, nullptr, DT3.p, G[b + 10], G[b + 11], nullptr, nullptr, pxB};
            trunk_dgrad(ex, g.res_out[i], packed, DH, DT2, 0, nullptr, &pa);
            TrunkPre pb{2, res(i, R_CA).p, res(i, R_SA).p, P[b + 2], P[b + 3], P[b + 6], P[b + 7], DT1.p, G[b + 2], G[b + 3], G[b + 6], G[b + 7], pxB};
            ns = 1;
            trunk_dgrad(ex, g.res_vg[i], packed, DT2, DH, 1, &ns, &pb);
            if (batch_w) queue_wgrads(i, hin, DT3, DT1);
            else {
                conv_wgrad(ex, g.res_out[i], G, res(i, R_YA).image(), DT3.image());
                conv_wgrad(ex, g.res_vg[i], G, hin.image(), DT1.image());
            }
            continue;
        }
        norm_bwd(ex, res(i, R_CB), normp(P, G, b + 10, b + 11), res(i, R_SB).p, DH, ns, DT3, 0, ACT_NONE);
        int ns2 = 1;
        conv_wgrad(ex, g.res_out[i], G, res(i, R_YA).image(), DT3.image());
        if (!trunk_dgrad(ex, g.res_out[i], packed, DT3, DT2, 0))
            conv_dgrad(ex, g.res_out[i], packed, DT3.image(), DT2.image(), 0, 1, &ns2);
        norm_bwd(ex, res(i, R_CA), normp(P, G, b + 2, b + 3, b + 6, b + 7), res(i, R_SA).p, DT2, ns2, DT1, 0, ACT_GLU);
        conv_wgrad(ex, g.res_vg[i], G, hin.image(), DT1.image());
        ns = 1;          // (deterministic mode: DH is left alone and its K-split partials go to slabs the next norm_bwd sums)
        if (!trunk_dgrad(ex, g.res_vg[i], packed, DT1, DH, 1 /*accumulate: skip path*/, &ns))
            conv_dgrad(ex, g.res_vg[i], packed, DT1.image(), DH.image(), 1, 1, &ns);      // (a K split leaves its partials in slabs the next norm_bwd sums)
    }
    // ONE launch for the residual layers' weight gradients, beside the rest of the backward chain
    if (nwjobs > 0) ex.fail(mcvc_wgrad_smallk_batch_launch(wjobs, nwjobs, B, W4, fork_aux(ex)));
    if (milestones) record_milestone(ex, milestones[1]);          // parameters [24,100) are done
    // ---- conv2dto1d + IN (:254-255)
    const Tensor dy4 = DT3s[1], dy3 = q.trunk(GA, 0, 5120);
    norm_bwd(ex, o[GS_C4], normp(P, G, 22, 23), o[GS_S4].p, DH, ns, dy4, 0, ACT_NONE);
    conv_wgrad(ex, g.c2d1d, G, o[GS_Y3].image(), dy4.image());
    ns = 1;
    if (!trunk_dgrad(ex, g.c2d1d, packed, dy4, dy3, 0))
        conv_dgrad(ex, g.c2d1d, packed, dy4.image(), dy3.image(), 0, 1, &ns);
    // ---- downSample2 (:246): dy is in trunk layout
    GB = nextGB();
    norm_bwd(ex, o[GS_C3], normp(P, G, 14, 15, 18, 19), o[GS_S3].p, dy3.rows20(), ns, o[GS_C3].at(GB), 0, ACT_GLU);
    conv_wgrad(ex, g.ds2, G, o[GS_Y2], o[GS_C3].at(GB));
    conv_dgrad(ex, g.ds2, packed, o[GS_C3].at(GB), o[GS_Y2].at(GA), 0, 1, &ns);
    if (milestones && ex.fine_ms) record_milestone(ex, milestones[2]);          // parameters [12,24) (downSample2, conv2dto1d) are done
    // ---- downSample1 (:245)
    GB = nextGB();
    norm_bwd(ex, o[GS_C2], normp(P, G, 6, 7, 10, 11), o[GS_S2].p, o[GS_Y2].at(GA), ns, o[GS_C2].at(GB), 0, ACT_GLU);
    conv_wgrad(ex, g.ds1, G, o[GS_Y1], o[GS_C2].at(GB));
    conv_dgrad(ex, g.ds1, packed, o[GS_C2].at(GB), o[GS_Y1].at(GA), 0, 1, &ns);
    if (milestones && ex.fine_ms) record_milestone(ex, milestones[3]);          // parameters [4,12) (downSample1) are done
    // ---- conv1 gated GLU (:242)
    GB = nextGB();
    act_bwd(ex, o[GS_C1], o[GS_Y1].at(GA), ns, o[GS_C1].at(GB), ACT_GLU);
    ex.br1_on_main = (dx == nullptr) ? 1 : 0;
    conv_wgrad(ex, g.conv1, G, o[GS_XIN], o[GS_C1].at(GB));
    ex.br1_on_main = 0;
    conv_bias_grad(ex, g.conv1, G, o[GS_C1].at(GB));
    if (dx) {
        const Tensor dxin = o[GS_XIN].at(GA);
        conv_dgrad(ex, g.conv1, packed, o[GS_C1].at(GB), dxin, 0, 1, &ns);
        if (!ex.dry) ex.fail(mcvc_mask_grad_launch(GA, ex.slabs, dxin.dense(), ns, mask, dx, B, 80 * T, 2, accumulate_dx, ex.s));
    }
    if (ex.no_join) ex.readers.clear(); else join_aux(ex);
}

// =================================================================================================
// Discriminator
// =================================================================================================
struct DiscNet { ConvSpec conv1, ds[3], outc; long long packed_floats; };
static DiscNet build_disc()
{
    DiscNet n{};
    long long cur = 0;
    n.conv1 = mk(1, 128, 1, 3, 3, 1, 1, 1, 0, 1, -1, -1, 1);             // model.py:290-295
    n.ds[0] = mk(128, 256, 1, 3, 3, 2, 1, 1, 2, 3, -1, -1, 0);           // :298-302
    n.ds[1] = mk(256, 512, 1, 3, 3, 2, 1, 1, 6, 7, -1, -1, 0);           // :304-308
    n.ds[2] = mk(512, 1024, 1, 3, 3, 2, 1, 1, 10, 11, -1, -1, 0);        // :310-314
    n.outc = mk(1024, 1, 1, 1, 3, 1, 0, 1, 18, 19, -1, -1, 1);           // :323-327   (downSample4, params 14-17, is dead: :316-320 never called)
    ConvSpec* all[] = {&n.conv1, &n.ds[0], &n.ds[1], &n.ds[2], &n.outc};
    int k = 0;
    for (ConvSpec* c : all) { c->index = k++; spec_finalize(*c, cur); }
    n.packed_floats = cur;
    return n;
}
static const DiscNet& disc_net() { static const DiscNet n = build_disc(); return n; }
static const ConvSpec* const* disc_specs()
{
    static const DiscNet& n = disc_net();
    static const ConvSpec* const v[] = {&n.conv1, &n.ds[0], &n.ds[1], &n.ds[2], &n.outc};
    return v;
}

struct DiscDims { int B, T, H[4], W[4]; long long big; };
static DiscDims disc_dims(int B, int T)
{
    DiscDims d{};
    d.B = B; d.T = T; d.H[0] = 80; d.W[0] = T;
    for (int i = 1; i < 4; ++i) { d.H[i] = conv_out(d.H[i - 1], 3, 2, 1); d.W[i] = conv_out(d.W[i - 1], 3, 2, 1); }
    d.big = (long long)B * 128 * 80 * T;
    // (gradient ping-pong buffers also hold dY in the padded layout of the implicit data gradient: (OH + 1) x (OW + 4) per plane)
    for (int i = 1; i < 4; ++i) { const long long p = (long long)B * (128 << i) * mcvc_dyp_plane(d.H[i], d.W[i]); if (p > d.big) d.big = p; }
    return d;
}

// the discriminator's stash (see the generator's): level l = the l-th stride-2 layer; the inputs of those layers -- y0, y of levels 0 and 1 --
// may be stored phase-split; the pass's input is copied behind the rest (the first layer's weight gradient reads it)
enum DiscStashId { DS_C0, DS_Y0, DS_LEVEL,                  // three levels of three rows: DS_LEVEL + 3 * l + L_*
                   DS_LOGIT = DS_LEVEL + 9, DS_XIN, DS_ROWS };
enum { L_C, L_S, L_Y };
struct DiscStashRow { int C, level; StashKind kind; };      // level: which of DiscDims' H[] x W[] planes
static const DiscStashRow kDiscStash[DS_ROWS] = {
    {128, 0, SK_BATCH}, {128, 0, SK_SPLIT},
    {256, 1, SK_BATCH}, {256, 1, SK_STATS}, {256, 1, SK_SPLIT},
    {512, 2, SK_BATCH}, {512, 2, SK_STATS}, {512, 2, SK_SPLIT},
    {1024, 3, SK_BATCH}, {1024, 3, SK_STATS}, {1024, 3, SK_BATCH},
    {1, 3, SK_BATCH}, {1, 0, SK_BATCH},
};
// the first (one input channel) and the output (one output channel) layer on their own kernels (fewout_kernels.hip) instead of the generic
// conv + activation pairs
static int disc_out_direct()
{
    static const int en = mcvc_knob("MCVC_DISC_OUT", 1);
    return en;
}

// every stride-2 layer of a (B, T) pass takes the implicit-GEMM kernels (and the first layer its own kernel, which stores the phase-split layout)
static bool disc_igemm(const DiscDims& d)
{
    const DiscNet& n = disc_net();
    bool ok = disc_out_direct() != 0;
    for (int i = 0; i < 3 && ok; ++i) ok = igemm_applies(n.ds[i], d.H[i], d.W[i]);
    return ok;
}

static Stash disc_stash(float* base, const DiscDims& d)
{
    StashRow rows[DS_ROWS];
    for (int i = 0; i < DS_ROWS; ++i) { const DiscStashRow& r = kDiscStash[i]; rows[i] = StashRow{r.C, d.H[r.level], d.W[r.level], r.kind}; }
    return stash_layout(rows, DS_ROWS, base, d.B, d.B, 0, disc_igemm(d));
}
struct DiscScratch { long long ga, gb, gb2, slabs; };
static DiscScratch disc_scratch(const DiscDims& d)
{
    DiscScratch s{};
    s.ga = 0; s.gb = (d.big + 3) & ~3LL; s.gb2 = 2 * s.gb; s.slabs = 3 * s.gb;
    return s;
}

static void disc_forward_impl(Exec& ex, const float* const* P, const float* packed, const float* x, float* out, float* st, const DiscDims& d)
{
    ex.params = P;
    const DiscNet& n = disc_net();
    const Stash o = disc_stash(st, d);
    const int B = d.B, T = d.T;
    int ns = 1;
    const bool ig = disc_igemm(d);           // the three stride-2 layers as implicit GEMMs: their inputs are stored phase-split (sgemm.h)
    // model.py:343-344  unsqueeze(1) -> conv 3x3 -> x*sigmoid(x)
    if (disc_out_direct() && !ex.dry) {
        ex.fail(mcvc_disc_conv1_fwd_launch(x, P[n.conv1.wi[0]], P[n.conv1.bi[0]], o[DS_C0].p, o[DS_Y0].p, B, 128, 80, T, ex.s, ig ? 1 : 0));
    } else {
        conv_fwd(ex, n.conv1, packed, nchw(x, B, 1, 80, T), o[DS_C0], 0, 1, &ns);
        act_fwd(ex, o[DS_C0], ns, o[DS_Y0], ACT_SILU);
    }
    const Tensor* h = &o[DS_Y0];
    for (int i = 0; i < 3; ++i) {                       // :345-347  (a level's y is phase-split when it feeds the next stride-2 layer)
        const Tensor* l = &o[DS_LEVEL + 3 * i];
        if (ig) conv_fwd_igemm(ex, n.ds[i], packed, *h, l[L_C], 1, &ns);
        else conv_fwd(ex, n.ds[i], packed, *h, l[L_C], 0, 1, &ns);
        norm_fwd(ex, l[L_C], ns, normp(P, nullptr, 4 + 4 * i, 5 + 4 * i), l[L_S].p, l[L_Y], nullptr, ACT_SILU);
        h = &l[L_Y];
    }
    // :348  1x3 conv to one channel + sigmoid
    const int H3 = d.H[3], W3 = d.W[3];
    if (disc_out_direct() && !ex.dry) {
        ex.fail(mcvc_disc_out_fwd_launch(h->p, P[n.outc.wi[0]], P[n.outc.bi[0]], o[DS_LOGIT].p, out, B, 1024, H3, W3, ex.s));
        return;
    }
    conv_fwd(ex, n.outc, packed, *h, o[DS_LOGIT], 0, 1, &ns);
    act_fwd(ex, o[DS_LOGIT], ns, o[DS_LOGIT].at(out), ACT_SIGMOID);
}

static void disc_backward_impl(Exec& ex, const float* const* P, const float* packed, float* const* G, const float* dout, int is_logit_grad,
                               float* dx, int accumulate_dx, const float* stc, float* sc, const DiscDims& d)
{
    ex.params = P;
    const DiscNet& n = disc_net();
    const Stash o = disc_stash(const_cast<float*>(stc), d);
    const DiscScratch q = disc_scratch(d);
    const int B = d.B, T = d.T;
    float* GA = sc + q.ga;
    float* GBs[2] = {sc + q.gb, sc + q.gb2};
    int gbi = 0;
    auto nextGB = [&]() { gbi ^= 1; return GBs[gbi]; };
    float* GB = GBs[0];
    const int H3 = d.H[3], W3 = d.W[3];
    int ns = 1;
    const float* dlogit = dout;
    if (!is_logit_grad) {                         // sigmoid backward (model.py:348)
        if (!ex.dry) ex.fail(mcvc_copy_launch(dout, GA, B * H3 * W3, ex.s));
        act_bwd(ex, o[DS_LOGIT], o[DS_LOGIT].at(GA), 1, o[DS_LOGIT].at(GB), ACT_SIGMOID);
        dlogit = GB;
    }
    const Tensor& y2 = o[DS_LEVEL + 6 + L_Y];
    const CTensor dlv = nchw(dlogit, B, 1, H3, W3);
    conv_wgrad(ex, n.outc, G, y2, dlv);
    conv_bias_grad(ex, n.outc, G, dlv);
    if (disc_out_direct() && !ex.dry) ex.fail(mcvc_disc_out_dgrad_launch(dlogit, P[n.outc.wi[0]], GA, B, 1024, H3, W3, ex.s));
    else conv_dgrad(ex, n.outc, packed, dlv, y2.at(GA), 0, 1, &ns);
    const bool ig = disc_igemm(d);
    for (int i = 2; i >= 0; --i) {
        const Tensor* l = &o[DS_LEVEL + 3 * i];
        const Tensor& hin = (i == 0) ? o[DS_Y0] : o[DS_LEVEL + 3 * (i - 1) + L_Y];
        GB = nextGB();
        // implicit GEMMs: dY leaves the InstanceNorm backward in the padded layout the data gradient gathers from (zero column / row written
        // there); the layer's input is stored phase-split (forward): the weight gradient's staging reads both as they are
        const Tensor dyv = ig ? padded_dy(GB, B, l[L_C].C, l[L_C].H, l[L_C].W) : l[L_C].at(GB);
        const Tensor dxv = nchw(GA, B, hin.C, hin.H, hin.W);
        norm_bwd(ex, l[L_C], normp(P, G, 4 + 4 * i, 5 + 4 * i), l[L_S].p, l[L_C].at(GA), ns, dyv, 0, ACT_SILU);
        conv_wgrad(ex, n.ds[i], G, hin, dyv);
        if (ig) conv_dgrad_igemm(ex, n.ds[i], packed, dyv, dxv, 0, 1, &ns);
        else conv_dgrad(ex, n.ds[i], packed, dyv, dxv, 0, 1, &ns);
    }
    GB = nextGB();
    act_bwd(ex, o[DS_C0], o[DS_C0].at(GA), ns, o[DS_C0].at(GB), ACT_SILU);
    conv_wgrad(ex, n.conv1, G, o[DS_XIN], o[DS_C0].at(GB));          // (the forward entry's copy of the input)
    conv_bias_grad(ex, n.conv1, G, o[DS_C0].at(GB));
    if (dx) {
        const Tensor dxin = o[DS_XIN].at(GA);
        conv_dgrad(ex, n.conv1, packed, o[DS_C0].at(GB), dxin, 0, 1, &ns);
        if (!ex.dry) ex.fail(mcvc_mask_grad_launch(GA, ex.slabs, dxin.dense(), ns, nullptr, dx, B, 80 * T, 1, accumulate_dx, ex.s));
    }
    join_aux(ex);
}

struct Needs { long long slab, wslab, sg, sgw; };

// split of the scratch tail into [conv slabs | wgrad slabs]: from a dry run of the schedule, cached per (net, B, T)
template <class F>
static Needs cached_needs(int kind, int B, int T, F&& dry_run)
{
    static std::mutex mu;
    static std::map<long long, Needs> cache;
    const long long key = ((long long)kind << 60) ^ ((long long)B << 32) ^ (long long)T;
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = cache.find(key);
        if (it != cache.end()) return it->second;
    }
    Exec ex{}; ex.dry = true;
    dry_run(ex);
    Needs n{(ex.slab_need + 3) & ~3LL, (ex.wslab_need + 3) & ~3LL, (ex.sg_need + 3) & ~3LL, (ex.sgw_need + 3) & ~3LL};
    std::lock_guard<std::mutex> lk(mu);
    cache[key] = n;
    return n;
}

static Exec make_exec(void* stream, void* aux_stream, float* scratch, long long scratch_floats, long long slab_off, const Needs& nd)
{
    Exec ex{};
    ex.s = (hipStream_t)stream; ex.s2 = (hipStream_t)aux_stream; ex.dry = false; ex.err = 0;
    ex.slabs = scratch + slab_off;
    ex.slab_cap = nd.slab;
    ex.sg = nd.sg ? scratch + slab_off + nd.slab : nullptr;
    ex.sg_cap = nd.sg;
    ex.sgw = nd.sgw ? scratch + slab_off + nd.slab + nd.sg : nullptr;
    ex.sgw_cap = nd.sgw;
    ex.wslabs = scratch + slab_off + nd.slab + nd.sg + nd.sgw;
    ex.wslab_cap = scratch_floats - slab_off - nd.slab - nd.sg - nd.sgw;
    return ex;
}

static Needs gen_needs(int B, int T)
{
    return cached_needs(1, B, T, [&](Exec& ex) {
        const GenDims d = gen_dims(B, T);
        gen_forward_impl(ex, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d);
        float dummy = 0.f;
        gen_backward_impl(ex, nullptr, nullptr, nullptr, nullptr, nullptr, &dummy, 0, nullptr, nullptr, d);
    });
}

static Needs disc_needs(int B, int T)
{
    return cached_needs(2, B, T, [&](Exec& ex) {
        const DiscDims d = disc_dims(B, T);
        disc_forward_impl(ex, nullptr, nullptr, nullptr, nullptr, nullptr, d);
        float dummy = 0.f;
        disc_backward_impl(ex, nullptr, nullptr, nullptr, nullptr, 1, &dummy, 0, nullptr, nullptr, d);
    });
}

}  // namespace

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int mcvc_version(void) { return MCVC_ABI_VERSION; }

// ---- grouped ("twin") launches (twin.h): the caller brackets two identical call sequences on different networks -------------------
static thread_local TwinCtx t_twin_ctx;
int mcvc_twin_begin(void)
{
    if (g_mcvc_twin) return MCVC_ERR_INVALID;
    t_twin_ctx.recs.clear(); t_twin_ctx.args.clear(); t_twin_ctx.next = 0; t_twin_ctx.err = 0; t_twin_ctx.phase = 1;
    g_mcvc_twin = &t_twin_ctx;
    return 0;
}
int mcvc_twin_switch(void)
{
    if (!g_mcvc_twin || g_mcvc_twin->phase != 1) return MCVC_ERR_INVALID;
    g_mcvc_twin->phase = 2;
    g_mcvc_twin->next = 0;
    return g_mcvc_twin->err;
}
int mcvc_twin_end(void)
{
    if (!g_mcvc_twin) return MCVC_ERR_INVALID;
    TwinCtx* t = g_mcvc_twin;
    g_mcvc_twin = nullptr;
    const int phase = t->phase;
    t->phase = 0;
    if (t->err) return t->err;
    if (phase != 2 || t->next != t->recs.size()) return MCVC_ERR_INVALID;     // the second walk issued fewer launches than the first
    return 0;
}
int mcvc_twin_launches(void) { return (int)t_twin_ctx.recs.size(); }

int mcvc_set_deterministic(int on) { const int was = g_deterministic; g_deterministic = on ? 1 : 0; return was; }
int mcvc_get_deterministic(void) { return g_deterministic; }
int mcvc_set_precise(int on) { const int was = g_precise; g_precise = on ? 1 : 0; return was; }
int mcvc_get_precise(void) { return g_precise; }
int mcvc_set_trunk_persistent(int on) { const int was = g_trunk_net; g_trunk_net = (on == 2) ? 2 : (on ? 1 : 0); return was; }

long long mcvc_gen_packed_floats(void) { return gen_net().packed_floats; }
long long mcvc_disc_packed_floats(void) { return disc_net().packed_floats; }
int mcvc_gen_out_frames(int T) { return gen_dims(1, T).Wu2; }
int mcvc_disc_out_frames(int T) { return disc_dims(1, T).W[3]; }

long long mcvc_gen_stash_floats(int B, int T) { return gen_stash(nullptr, gen_dims(B, T), B).total; }

long long mcvc_gen_scratch_floats(int B, int T)
{
    const Needs nd = gen_needs(B, T);
    return gen_scratch(gen_dims(B, T)).slabs + nd.slab + nd.sg + nd.sgw + nd.wslab + 64;
}

long long mcvc_disc_stash_floats(int B, int T)
{
    return disc_stash(nullptr, disc_dims(B, T)).total;          // (with the copy of the input for the first layer's weight gradient)
}

long long mcvc_disc_scratch_floats(int B, int T)
{
    const Needs nd = disc_needs(B, T);
    return disc_scratch(disc_dims(B, T)).slabs + nd.slab + nd.sg + nd.sgw + nd.wslab + 64;
}

// every form of every layer, in layer order
static PackPlan full_plan(int net, const ConvSpec* const* specs, int nlayers)
{
    PackPlan k;
    k.net = net;
    for (int l = 0; l < nlayers; ++l) k.add(*specs[l], kAllForms);
    return k;
}
static int pack_plan_run(const PackPlan& k, const ConvSpec* const* specs, const float* const* params, float* packed, void* stream)
{
    int err = 0;
    const DevPackTable* t = dev_pack_table(k, specs, &err);
    if (!t) return err ? err : MCVC_ERR_INVALID;
    record_fresh(packed, k);
    if (t->njobs == 0) return 0;
    return pack_net(t, params, packed, (hipStream_t)stream);
}

int mcvc_gen_pack(const float* const* params, float* packed, void* stream)
{
    return pack_plan_run(full_plan(0, gen_specs(), kMaxLayers), gen_specs(), params, packed, stream);
}

// 1 if every 1-D layer of a generator pass with batch B at T frames takes the fused trunk path (see trunk_fwd / trunk_dgrad)
int mcvc_gen_trunk_fused(int B, int T)
{
    if (B < 1 || T < 1 || !trunk_enabled()) return 0;
    const GenNet& g = gen_net();
    const GenDims d = gen_dims(B, T);
    const int W4 = d.W4;
    bool ok = true;
    for (int i = 0; i < 6 && ok; ++i) {
        ok = ok && mcvc_trunk_applies(g.res_vg[i].Cin, 3, g.res_vg[i].Cout, B, W4, TRUNK_IN_GLU, 1);
        ok = ok && mcvc_trunk_applies(g.res_out[i].Cin, 3, g.res_out[i].Cout, B, W4, TRUNK_IN, 1);
        ok = ok && mcvc_trunk_applies(g.res_out[i].cout_tot, 3, g.res_out[i].Cin, B, W4, TRUNK_PLAIN, 1);
        ok = ok && trunk_pick_ksplit(g.res_vg[i].cout_tot, 3, g.res_vg[i].Cin, B, W4, 0) >= 1;
    }
    ok = ok && mcvc_trunk_applies(g.c1d2d.Cin, 1, g.c1d2d.Cout, B, W4, TRUNK_IN, 1);
    ok = ok && trunk_pick_ksplit(g.c1d2d.cout_tot, 1, g.c1d2d.Cin, B, W4, 0) >= 1;       // its data-gradient (K = 5120)
    ok = ok && trunk_pick_ksplit(g.c2d1d.Cin, 1, g.c2d1d.Cout, B, W4, 1) >= 1;           // conv2dto1d forward (K = 5120)
    ok = ok && mcvc_trunk_applies(g.c2d1d.cout_tot, 1, g.c2d1d.Cin, B, W4, TRUNK_PLAIN, 1);
    return ok ? 1 : 0;
}

// bit 0: the persistent forward trunk kernel would run a (B, T) pass, bit 1: the persistent backward -- under the current switches
// (mcvc_set_trunk_persistent) and the residency bound (mcvc_set_trunk_passes_in_flight x 64 workgroups <= compute units)
int mcvc_gen_trunk_persistent(int B, int T)
{
    if (B < 1 || T < 1 || !trunk_enabled()) return 0;
    const int W4 = gen_dims(B, T).W4;
    int m = 0;
    if (trunk_net_enabled() && mcvc_trunk_net_applies(B, W4)) m |= 1;
    if (trunk_bwd_net_enabled() && mcvc_trunk_bwd_net_applies(B, W4)) m |= 2;
    return m;
}

// `sets`: 1 = only what a forward pass reads, 2 = only what a backward pass reads, 3 = both (PackSide).  After a forward-only
// refresh no backward form of the layers is fresh and a backward pass on this buffer fails until sets = 2 has run.
int mcvc_gen_pack_sets(const float* const* params, float* packed, int max_batch, int T, int sets, void* stream)
{
    return mcvc_gen_pack_ranges(params, packed, max_batch, T, sets, 7, stream);
}

// ... restricted to the layers of some parameter ranges (bit 0: upSample1/2 + lastConvLayer = parameters [100,110); bit 1: the residual
// blocks + conv1dto2d = [24,100); bit 2: conv1, downSample1/2, conv2dto1d = [0,24) -- the ranges whose gradients become final one after the
// other during a backward pass, mcvc_gen_backward_overlap): the optimizer step + re-pack of a range can then run beside the rest of the pass
struct GenPackCfg { bool fused, wino_only, w4, w43, up1_w4, up1_w2, up2_w2; };
static GenPackCfg gen_pack_cfg(int max_batch, int T)
{
    GenPackCfg q{};
    q.fused = true;
    for (int b = 1; b <= max_batch; ++b)
        if (!mcvc_gen_trunk_fused(b, T)) q.fused = false;
    // every 5x5 layer of every such pass runs on the Winograd kernels (conv_wino / the wino3 branches take no fallback) when
    // the frame count keeps all image sizes even, the tile counts are inside the kernels' range and nothing was switched
    // off through the MCVC_WINO* knobs: then their direct K-major copies are not refreshed either
    static const bool knobs_default = !mcvc_knob_set("MCVC_WINO") && !mcvc_knob_set("MCVC_WINO3") && !mcvc_knob_set("MCVC_WINO3_FWD") && !mcvc_knob_set("MCVC_WINO_GEMM");
    const GenDims dm = gen_dims(max_batch, T);
    const bool wino_default = knobs_default && !g_precise;
    q.wino_only = q.fused && wino_default && (T % 4) == 0 && T >= 32 && (long long)max_batch * 20 * dm.W4 <= 16384;
    // the 64-point weight sets of upSample1/2 only when some pass can take the F(4x4,5x5) path (wino4_applies); otherwise not written
    q.w4 = wino_default && wino4_min_nb() > 0 && max_batch >= wino4_min_nb() && (T % 16) == 0;
    q.w43 = wino_default && wino43_min_nb() > 0 && max_batch >= wino43_min_nb() && (T % 16) == 0;
    q.up1_w4 = (long long)max_batch * 5 * (T / 16) >= wino4_min_tiles();             // upSample1 runs on 20 x T/4 images: 5 x T/16 tiles per sample
    // the 36-point sets of a layer only where some pass still runs F(2x2,5x5): a layer with >= wino4_min_tiles() tiles PER SAMPLE (upSample2
    // at 64 frames: 80) takes the 4 x 4 scheme in every pass, forward, data gradient and weight gradient (wino4_applies), so its 36-point
    // sets -- 2 x 36/25 of its weights per step -- have no reader (r5)
    const bool all4 = q.w4 && wino4_min_nb() == 1;
    q.up1_w2 = !(all4 && 5LL * (T / 16) >= wino4_min_tiles());
    q.up2_w2 = !(all4 && 10LL * (T / 8) >= wino4_min_tiles());
    return q;
}
// range_mask bits: 1 = parameters [100,110), 2 = [24,100), 4 = [0,24); r4: the head in three parts, in the order their gradients become final
// during a backward pass (MCVC_BWD_FINE_MILESTONES): 8 = [12,24) (downSample2, conv2dto1d), 16 = [4,12) (downSample1), 32 = [0,4) (conv1)
static bool gen_range_mask_ok(int m) { return m >= 1 && m <= 63 && !((m & 4) && (m & 56)); }
static bool gen_in_range(int m, int p)
{
    return ((m & 1) && p >= 100 && p < 110) || ((m & 2) && p >= 24 && p < 100) || ((m & 4) && p < 24) ||
           ((m & 8) && p >= 12 && p < 24) || ((m & 16) && p >= 4 && p < 12) || ((m & 32) && p < 4);
}
static PackPlan gen_pack_build(const GenPackCfg& q, int sets, int range_mask, int update)
{
    const GenNet& g = gen_net();
    PackPlan k;
    k.net = 0; k.update = update; k.sets = sets;
    const unsigned w4 = form_bit(PF_W4F) | form_bit(PF_W4D), w43 = form_bit(PF_W43F) | form_bit(PF_W43D), w2 = form_bit(PF_W2F) | form_bit(PF_W2D);
    auto conv2d = [&](const ConvSpec& c, bool c_w4, bool c_w2) {
        k.add(c, (q.wino_only ? wino_only_forms(c) : kAllForms) & ~((c_w4 ? 0 : w4) | (q.w43 ? 0 : w43) | (c_w2 ? 0 : w2)));
    };
    auto trunk = [&](const ConvSpec& c) { k.add(c, q.fused ? trunk_fused_forms(c) : kAllForms); };
    if (range_mask & (4 | 32)) conv2d(g.conv1, q.w4, true);
    if (range_mask & (4 | 16)) conv2d(g.ds1, q.w4, true);
    if (range_mask & (4 | 8)) { conv2d(g.ds2, q.w4, true); trunk(g.c2d1d); }
    if (range_mask & 1) {
        // (a layer whose largest pass has fewer than 64 F(4x4) tiles never takes that path, conv_wino4: its 64-point sets are not written)
        conv2d(g.up1, q.w4 && q.up1_w4, q.up1_w2);
        conv2d(g.up2, q.w4, q.up2_w2);
        conv2d(g.last, q.w4, true);
    }
    if (range_mask & 2) {
        trunk(g.c1d2d);
        for (int i = 0; i < 6; ++i) { trunk(g.res_vg[i]); trunk(g.res_out[i]); }
    }
    return k;
}

int mcvc_gen_pack_ranges(const float* const* params, float* packed, int max_batch, int T, int sets, int range_mask, void* stream)
{
    if (sets < 1 || sets > 3 || !gen_range_mask_ok(range_mask)) return MCVC_ERR_INVALID;
    return pack_plan_run(gen_pack_build(gen_pack_cfg(max_batch, T), sets, range_mask, 0), gen_specs(), params, packed, stream);
}

// optimizer.step() of a generator's parameter ranges (train.py:242) fused with the refresh of every packed copy derived from them: ONE
// launch, one reader and one writer per weight (update_net_kernel).  `numel`: element count of each of the 110 parameter tensors;
// flat / grad / grad2 (nullable) / exp_avg / exp_avg_sq: the flat buffers the parameters, their gradients and moments live in at EQUAL
// offsets (the engine's layout): the gradient of params[i] is grad + (params[i] - flat).  zero_grads: clear the gradient(s) behind the read.
int mcvc_gen_update_ranges(const float* const* params, const long long* numel, float* packed, int max_batch, int T, int range_mask,
                           const float* flat, float* grad, float* grad2, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
                           float eps, int step, float grad_scale, int zero_grads, void* stream)
{
    if (!params || !numel || !packed || !gen_range_mask_ok(range_mask)) return MCVC_ERR_INVALID;
    const PackPlan k = gen_pack_build(gen_pack_cfg(max_batch, T), 3, range_mask, 1);
    int err = MCVC_ERR_INVALID;
    std::vector<char> in_range(MCVC_GEN_NPARAMS);
    for (int p = 0; p < MCVC_GEN_NPARAMS; ++p) in_range[p] = gen_in_range(range_mask, p);
    const DevUpdTable* t = dev_upd_table(k, gen_specs(), numel, MCVC_GEN_NPARAMS, in_range, &err);
    if (!t) return err;
    record_fresh(packed, k);          // (a range's update leaves the forms of ITS layers fresh)
    return update_net(t, params, numel, packed, UpdOpt{flat, grad, grad2, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, grad_scale, zero_grads}, (hipStream_t)stream);
}

int mcvc_gen_pack_small_batch(const float* const* params, float* packed, int max_batch, int T, void* stream)
{
    return mcvc_gen_pack_sets(params, packed, max_batch, T, 3, stream);
}

int mcvc_disc_pack(const float* const* params, float* packed, void* stream)
{
    return pack_plan_run(full_plan(1, disc_specs(), 5), disc_specs(), params, packed, stream);
}

// Discriminator re-pack restricted to what the implicit-GEMM schedule reads: of the three stride-2 layers (99.9 % of the weights) only the
// tap-major FORWARD copy + bias -- it serves the forward pass and, read row-major, the data gradient (sgemm.h arow); the weight gradient reads
// no weights at all; the first / output layers (tiny) are refreshed in full.  Falls back to the full pack when a layer would not take that
// path at T frames.  The direct kernels' copies of those layers are then not fresh and refuse to run.
int mcvc_disc_pack_small(const float* const* params, float* packed, int T, void* stream) { return mcvc_disc_pack_batch(params, packed, 1, T, stream); }

// which job table a discriminator re-pack for passes of up to max_batch samples uses: 1 = full, 4 = implicit GEMMs
static int disc_pack_kind(int max_batch, int T)
{
    return disc_igemm(disc_dims(max_batch < 1 ? 1 : max_batch, T)) ? 4 : 1;
}
static PackPlan disc_pack_build(int kind, int update)
{
    const DiscNet& n = disc_net();
    PackPlan k;
    k.net = 1; k.update = update;
    k.add(n.conv1, kAllForms);
    for (int i = 0; i < 3; ++i) k.add(n.ds[i], kind == 1 ? kAllForms : igemm_only_forms(n.ds[i]));
    k.add(n.outc, kAllForms);
    return k;
}

int mcvc_disc_pack_batch(const float* const* params, float* packed, int max_batch, int T, void* stream)
{
    return pack_plan_run(disc_pack_build(disc_pack_kind(max_batch, T), 0), disc_specs(), params, packed, stream);
}

// optimizer.step() of one discriminator (train.py:299) fused with the refresh of its packed copies; arguments as mcvc_gen_update_ranges
// (`numel`: 20 entries, 0 for the parameters of the unused downSample4 block, which are neither updated nor packed).
int mcvc_disc_update_batch(const float* const* params, const long long* numel, float* packed, int max_batch, int T,
                           const float* flat, float* grad, float* grad2, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
                           float eps, int step, float grad_scale, int zero_grads, void* stream)
{
    if (!params || !numel || !packed) return MCVC_ERR_INVALID;
    const PackPlan k = disc_pack_build(disc_pack_kind(max_batch, T), 1);
    int err = MCVC_ERR_INVALID;
    const DevUpdTable* t = dev_upd_table(k, disc_specs(), numel, MCVC_DISC_NPARAMS, std::vector<char>(MCVC_DISC_NPARAMS, 1), &err);
    if (!t) return err;
    record_fresh(packed, k);
    return update_net(t, params, numel, packed, UpdOpt{flat, grad, grad2, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, grad_scale, zero_grads}, (hipStream_t)stream);
}

// ---- host view of a pack / update plan (no device call): one row of kPlanW 64-bit integers per record (include/mcvc.h) ---------------------
namespace {
constexpr int kPlanW = 20, kLayoutW = 12;
struct PlanRows {
    long long* rows; int cap, w = kPlanW, n = 0;
    void put(std::initializer_list<long long> v)
    {
        if (n < cap) { long long* r = rows + (long long)n * w; int i = 0; for (long long x : v) r[i++] = x; for (; i < w; ++i) r[i] = 0; }
        ++n;
    }
};
static long long dbits(double d) { long long b; memcpy(&b, &d, sizeof(b)); return b; }
// element counts of a network's parameter tensors: the convolutions' from their specs, the norm affine pairs that follow a convolution
static void net_numel(const ConvSpec* const* specs, int n, long long* numel)
{
    for (int l = 0; l < n; ++l) {
        const ConvSpec& c = *specs[l];
        const bool edge = l == 0 || c.Cout == 1;                        // conv1 / the last layer: no norm behind them
        for (int br = 0; br < c.nbr; ++br) {
            numel[c.wi[br]] = (long long)c.Cout * c.Cin * c.KH * c.KW; numel[c.bi[br]] = c.Cout;
            if (!edge) numel[c.wi[br] + 2] = numel[c.wi[br] + 3] = c.wino ? c.Cout / 4 : c.Cout;      // (upSample1/2: PixelShuffle(2) before the norm)
        }
    }
}
}  // namespace

int mcvc_pack_plan(int net, int max_batch, int T, int sets, int range_mask, int update, long long* rows, int cap, int* n_rows)
{
    if (!n_rows || (net != 0 && net != 1) || (update != 0 && update != 1) || max_batch < 1 || T < 1 || sets < 1 || sets > 3 || (update && sets != 3) ||
        cap < 0 || (cap > 0 && !rows)) return MCVC_ERR_INVALID;
    if (net == 0 ? !gen_range_mask_ok(range_mask) : range_mask != 7) return MCVC_ERR_INVALID;
    const ConvSpec* const* specs = net == 0 ? gen_specs() : disc_specs();
    const int nl = net == 0 ? kMaxLayers : 5, nparams = net == 0 ? MCVC_GEN_NPARAMS : MCVC_DISC_NPARAMS;
    long long cfg = 0;
    PackPlan k;
    if (net == 0) {
        const GenPackCfg q = gen_pack_cfg(max_batch, T);
        cfg = q.fused | q.wino_only << 1 | q.w4 << 2 | q.w43 << 3 | q.up1_w4 << 4 | q.up1_w2 << 5 | q.up2_w2 << 6;
        k = gen_pack_build(q, sets, range_mask, update);
    } else {
        cfg = disc_pack_kind(max_batch, T);
        k = disc_pack_build((int)cfg, update);
    }
    const PackTable t = build_table(k, specs);
    UpdPlan u;
    if (update) {
        long long numel[128] = {};
        net_numel(specs, nl, numel);
        std::vector<char> in_range(nparams, 1);
        if (net == 0) for (int p = 0; p < nparams; ++p) in_range[p] = gen_in_range(range_mask, p);
        if (int e = plan_upd(t, numel, nparams, in_range, covered_params(k, specs), u)) return e;
    }
    const std::vector<PackJob>& jobs = update ? u.jobs : t.jobs;
    PlanRows R{rows, cap};
    R.put({0, net, update, (long long)jobs.size(), (long long)u.owners.size(), (long long)t.dga.size(), update ? u.nblocks : t.nblocks,
           net == 0 ? gen_net().packed_floats : disc_net().packed_floats, dbits(t.bytes), dbits(t.wbytes), cfg, kPlanW});
    for (const PackJob& j : jobs) {
        int layer = -1, form = -1;
        for (int l = 0; l < nl && layer < 0; ++l)          // whose form the job writes: the one of its kind that holds dst
            for (int f = 0; f < kNumForms; ++f) {
                const long long o = specs[l]->off[f];
                if (o >= 0 && kPackForms[f].kind == j.kind && j.dst >= o && j.dst < o + form_floats(*specs[l], (PackForm)f)) { layer = l; form = f; }
            }
        if (layer < 0) return MCVC_ERR_INVALID;
        const long long len = j.kind == PACK_COPY ? j.Cout : form_floats(*specs[layer], (PackForm)form);
        R.put({1, layer, form, j.kind, j.param, j.dst, len, j.block0, j.gx, j.Cout, j.Cin, j.K, j.ld, j.co_off, j.KW, j.taps, j.xi_stride, j.dg});
    }
    for (const UpdOwner& o : u.owners) R.put({2, o.param, o.block0, o.gx, o.Cout, o.Cin, o.taps, o.CB, o.IB, o.e0, o.ne, o.flat, o.vec4});
    std::sort(k.layers.begin(), k.layers.end());
    for (const auto& lf : k.layers) R.put({3, lf.first, sets, lf.second & side_forms(sets)});      // what record_fresh would note
    for (size_t i = 0; i < t.dga.size(); ++i) {
        const PackDgradArgs& a = t.dga[i];
        R.put({4, (long long)i, a.Cin, a.KH, a.KW, a.step, a.ld, a.co_off, a.merged, a.mg_kh, a.mg_kw, a.ncls, a.tapmajor, a.cout_rows});
        for (int c = 0; c < a.ncls; ++c) {
            const DgradClass& d = a.cls[c];
            R.put({5, (long long)i, c, d.nth, d.ntw, d.khmax, d.kwmax, d.pad_h, d.pad_w, d.qh, d.qw, d.su, d.sv, d.offset});
        }
    }
    *n_rows = R.n;
    return R.n > cap ? MCVC_ERR_WORKSPACE : 0;
}

// which parameter tensors a store pass covers (grad_store_covered; host only, no device call): covered[p] = 1 for the weight tensors of
// the covered layers, 0 for everything else; returns the network's parameter count
int mcvc_grad_store_mask(int net, int T, unsigned char* covered)
{
    if ((net != 0 && net != 1) || T < 1 || !covered) return MCVC_ERR_INVALID;
    memset(covered, 0, 128);
    const ConvSpec* const* specs = net == 0 ? gen_specs() : disc_specs();
    const int nl = net == 0 ? kMaxLayers : 5;
    for (int l = 0; l < nl; ++l) {
        const ConvSpec& c = *specs[l];
        if (!grad_store_covered(c)) continue;
        for (int br = 0; br < c.nbr; ++br) covered[c.wi[br]] = 1;
    }
    return net == 0 ? MCVC_GEN_NPARAMS : MCVC_DISC_NPARAMS;
}

// The stash and scratch layouts of a (B, T) pass as rows of kLayoutW integers (host only, no device call; include/mcvc.h)
int mcvc_net_layout(int net, int B, int T, int stash_B, int stash_b0, long long* rows, int cap, int* n_rows)
{
    if (!n_rows || (net != 0 && net != 1) || B < 1 || T < 1 || cap < 0 || (cap > 0 && !rows)) return MCVC_ERR_INVALID;
    if (stash_B < B) stash_B = B;
    if (stash_b0 < 0 || stash_b0 + B > stash_B || (net == 1 && stash_B != B)) return MCVC_ERR_INVALID;
    PlanRows R{rows, cap, kLayoutW};
    float* const base = nullptr;
    auto stash_rows = [&](const Stash& o) {
        for (int i = 0; i < o.n; ++i) { const Tensor& t = o[i]; R.put({1, R.n, o.off[i], o.floats[i], t.N, t.C, t.H, t.W, t.sb, t.sc, t.sh, o.win[i]}); }
    };
    auto raw = [&](long long off, long long n) { R.put({2, R.n, off, n, 0, 0, 0, 0, 0, 0, 0, off}); };
    Needs nd{};
    long long slabs = 0;
    if (net == 0) {
        const GenDims d = gen_dims(B, T);
        if (d.W4 < 2 || (stash_b0 > 0 && (((long long)stash_b0 * d.W4) & 3))) return MCVC_ERR_INVALID;
        stash_rows(gen_stash(base, d, stash_B, stash_b0));
        const GenScratch q = gen_scratch(d);
        auto grad = [&](long long off, int C) { const Tensor t = q.trunk(base, off, C); R.put({2, R.n, off, t.dense(), t.N, t.C, t.H, t.W, t.sb, t.sc, t.sh, off}); };
        const int nblk = mcvc_wgrad_smallk_batch_applies(B, d.W4) ? 6 : 0;
        raw(q.sync, 2 * MCVC_TRUNK_SYNC_WORDS); raw(q.ga, d.big); raw(q.gb, d.big); raw(q.gb2, d.big);
        grad(q.dh, 256); grad(q.dt1, 1024); grad(q.dt1b, 1024); grad(q.dt2, 512); grad(q.dt3, 256); grad(q.dt3b, 256);
        grad(q.dtx1, nblk * 1024); grad(q.dtx3, nblk * 256);
        raw(q.wv, q.wino_floats); raw(q.wm, q.wino_floats); raw(q.wv2, q.wino_floats); raw(q.wm2, q.wino_floats); raw(q.wu, q.wu_floats);
        nd = gen_needs(B, T); slabs = q.slabs;
    } else {
        const DiscDims d = disc_dims(B, T);
        stash_rows(disc_stash(base, d));
        const DiscScratch q = disc_scratch(d);
        for (long long off : {q.ga, q.gb, q.gb2}) raw(off, d.big);
        nd = disc_needs(B, T); slabs = q.slabs;
    }
    R.put({3, 0, nd.slab, nd.wslab, nd.sg, nd.sgw, slabs});
    *n_rows = R.n;
    return R.n > cap ? MCVC_ERR_WORKSPACE : 0;
}

int mcvc_gen_forward(const float* const* params, const float* packed, const float* x, const float* mask, float* out, float* stash,
                     float* scratch, long long scratch_floats, int B, int T, void* stream)
{
    if (B < 1 || T < 1 || !params || !packed || !x || !out || !stash || !scratch) return MCVC_ERR_INVALID;
    const GenDims d = gen_dims(B, T);
    if (d.W4 < 2) return MCVC_ERR_INVALID;        // T <= 4: the trunk's InstanceNorm1d would see one frame (the reference raises there too)
    Exec ex = make_exec(stream, nullptr, scratch, scratch_floats, gen_scratch(d).slabs, gen_needs(B, T));
    if (ex.wslab_cap < 0) return MCVC_ERR_WORKSPACE;
    { const GenScratch q = gen_scratch(d); ex.wv = scratch + q.wv; ex.wm = scratch + q.wm; ex.wino_cap = q.wino_floats;
      ex.sync = reinterpret_cast<unsigned*>(scratch + q.sync); }
    ex.fresh = get_fresh(packed);
    gen_forward_impl(ex, params, packed, x, mask, out, stash, d);
    return ex.err;
}

// Error word of the persistent trunk kernels in a generator scratch buffer (sticky until reset): 0 = no fault, 1 + l = a workgroup gave
// up waiting for the arrivals of layer l (the pass's output was poisoned with NaN).  SYNCHRONOUS (a 4-byte device-to-host copy on `stream`).
int mcvc_gen_trunk_fault(float* scratch, int B, int T, int reset, void* stream)
{
    if (!scratch || B < 1 || T < 1) return -MCVC_ERR_INVALID;
    unsigned* w = reinterpret_cast<unsigned*>(scratch + gen_scratch(gen_dims(B, T)).sync) + MCVC_TRUNK_SYNC_WORDS - 1;
    unsigned v = 0;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(&v, w, sizeof(v), hipMemcpyDeviceToHost, s) != hipSuccess) return -MCVC_ERR_INVALID;
    if (reset && hipMemsetAsync(w, 0, sizeof(v), s) != hipSuccess) return -MCVC_ERR_INVALID;
    if (hipStreamSynchronize(s) != hipSuccess) return -MCVC_ERR_INVALID;
    return (int)(v & 0x7fffffffu);             // (an un-initialised word -- first read after allocation -- must not look like an error return)
}
int mcvc_debug_trunk_fault_inject(int on) { return mcvc_trunk_set_fault_inject(on); }
int mcvc_set_trunk_passes_in_flight(int n) { return mcvc_trunk_set_passes_in_flight(n); }

int mcvc_gen_backward_overlap(const float* const* params, const float* packed, float* const* grads, const float* mask, const float* dout,
                              float* dx, int accumulate_dx, const float* stash, float* scratch, long long scratch_floats, int B, int T,
                              void* stream, void* aux_stream, void* const* milestones)
{
    return mcvc_gen_backward_flags(params, packed, grads, mask, dout, dx, accumulate_dx, stash, scratch, scratch_floats, B, T, stream, aux_stream,
                                   milestones, 0);
}

int mcvc_gen_backward_flags(const float* const* params, const float* packed, float* const* grads, const float* mask, const float* dout,
                            float* dx, int accumulate_dx, const float* stash, float* scratch, long long scratch_floats, int B, int T,
                            void* stream, void* aux_stream, void* const* milestones, int flags)
{
    return mcvc_gen_backward_window(params, packed, grads, mask, dout, dx, accumulate_dx, stash, B, 0, scratch, scratch_floats, B, T, stream, aux_stream,
                                    milestones, flags);
}

int mcvc_gen_backward_prefix(const float* const* params, const float* packed, float* const* grads, const float* mask, const float* dout,
                             float* dx, int accumulate_dx, const float* stash, int stash_B, float* scratch, long long scratch_floats, int B, int T,
                             void* stream, void* aux_stream, void* const* milestones, int flags)
{
    return mcvc_gen_backward_window(params, packed, grads, mask, dout, dx, accumulate_dx, stash, stash_B, 0, scratch, scratch_floats, B, T, stream,
                                    aux_stream, milestones, flags);
}

int mcvc_gen_backward_window(const float* const* params, const float* packed, float* const* grads, const float* mask, const float* dout,
                             float* dx, int accumulate_dx, const float* stash, int stash_B, int stash_b0, float* scratch, long long scratch_floats,
                             int B, int T, void* stream, void* aux_stream, void* const* milestones, int flags)
{
    if (B < 1 || T < 1 || stash_b0 < 0 || stash_B < stash_b0 + B || !params || !packed || !dout || !stash || !scratch) return MCVC_ERR_INVALID;
    const GenDims d = gen_dims(B, T);
    if (d.W4 < 2) return MCVC_ERR_INVALID;        // (as mcvc_gen_forward)
    Exec ex = make_exec(stream, aux_stream, scratch, scratch_floats, gen_scratch(d).slabs, gen_needs(B, T));
    if (ex.wslab_cap < 0) return MCVC_ERR_WORKSPACE;
    { const GenScratch q = gen_scratch(d); ex.wv = scratch + q.wv; ex.wm = scratch + q.wm; ex.wino_cap = q.wino_floats;
      ex.wv2 = scratch + q.wv2; ex.wm2 = scratch + q.wm2; ex.wu = scratch + q.wu; ex.wu_cap = q.wu_floats;
      ex.sync = reinterpret_cast<unsigned*>(scratch + q.sync); }
    ex.fresh = get_fresh(packed);
    for (int l = 0; l < kMaxLayers; ++l)          // forward-only re-pack of a layer: none of its backward forms is fresh (mcvc_gen_pack_sets)
        if (!(ex.fresh.layer[l] & spec_forms(*gen_specs()[l]) & side_forms(PACK_SIDE_BWD))) return MCVC_ERR_INVALID;
    ex.no_join = (flags & 1) && aux_stream;
    ex.fine_ms = (flags & 2) != 0;
    ex.store_grads = (flags & MCVC_BWD_STORE_GRADS) ? 1 : 0;
    gen_backward_impl(ex, params, packed, grads, mask, dout, dx, accumulate_dx, stash, scratch, d, milestones, stash_B, stash_b0);
    return ex.err;
}

int mcvc_gen_backward(const float* const* params, const float* packed, float* const* grads, const float* mask, const float* dout,
                      float* dx, int accumulate_dx, const float* stash, float* scratch, long long scratch_floats, int B, int T, void* stream,
                      void* aux_stream)
{
    return mcvc_gen_backward_overlap(params, packed, grads, mask, dout, dx, accumulate_dx, stash, scratch, scratch_floats, B, T, stream,
                                     aux_stream, nullptr);
}

int mcvc_disc_forward(const float* const* params, const float* packed, const float* x, float* out, float* stash, float* scratch,
                      long long scratch_floats, int B, int T, void* stream)
{
    if (B < 1 || T < 1 || !params || !packed || !x || !out || !stash || !scratch) return MCVC_ERR_INVALID;
    const DiscDims d = disc_dims(B, T);
    Exec ex = make_exec(stream, nullptr, scratch, scratch_floats, disc_scratch(d).slabs, disc_needs(B, T));
    if (ex.wslab_cap < 0) return MCVC_ERR_WORKSPACE;
    ex.fresh = get_fresh(packed);
    // keep the input for the first layer's weight gradient
    ex.fail(mcvc_copy_launch(x, disc_stash(stash, d)[DS_XIN].p, B * 80 * T, ex.s));
    disc_forward_impl(ex, params, packed, x, out, stash, d);
    return ex.err;
}

int mcvc_disc_backward(const float* const* params, const float* packed, float* const* grads, const float* dout, int dout_is_logit_grad,
                       float* dx, int accumulate_dx, const float* stash, float* scratch, long long scratch_floats, int B, int T, void* stream,
                       void* aux_stream)
{
    return mcvc_disc_backward_flags(params, packed, grads, dout, dout_is_logit_grad, dx, accumulate_dx, stash, scratch, scratch_floats, B, T, stream,
                                    aux_stream, 0);
}

int mcvc_disc_backward_flags(const float* const* params, const float* packed, float* const* grads, const float* dout, int dout_is_logit_grad,
                             float* dx, int accumulate_dx, const float* stash, float* scratch, long long scratch_floats, int B, int T, void* stream,
                             void* aux_stream, int flags)
{
    if (flags & ~MCVC_BWD_STORE_GRADS) return MCVC_ERR_INVALID;
    if (B < 1 || T < 1 || !params || !packed || !dout || !stash || !scratch) return MCVC_ERR_INVALID;
    const DiscDims d = disc_dims(B, T);
    Exec ex = make_exec(stream, aux_stream, scratch, scratch_floats, disc_scratch(d).slabs, disc_needs(B, T));
    if (ex.wslab_cap < 0) return MCVC_ERR_WORKSPACE;
    ex.fresh = get_fresh(packed);
    ex.store_grads = (flags & MCVC_BWD_STORE_GRADS) ? 1 : 0;
    disc_backward_impl(ex, params, packed, grads, dout, dout_is_logit_grad, dx, accumulate_dx, stash, scratch, d);
    return ex.err;
}

int mcvc_l1_loss(const float* a, const float* b, long long n, float weight, float* loss_slot, float* term_slot, float* grad_a,
                 int accumulate_grad, void* stream)
{
    return mcvc_l1_loss_launch(a, b, n, weight, loss_slot, term_slot, grad_a, accumulate_grad, (hipStream_t)stream);
}

int mcvc_loss_combine(const float* pairs, int n, const int* loss_dst, const int* term_dst, float* slots, void* stream)
{
    if (!pairs || !slots || !loss_dst || !term_dst) return MCVC_ERR_INVALID;
    return mcvc_loss_combine_launch(pairs, n, loss_dst, term_dst, slots, (hipStream_t)stream);
}

int mcvc_lsgan_loss(const float* d, long long n, float target, float weight, float* loss_slot, float* term_slot, float* grad_logit, void* stream)
{
    return mcvc_lsgan_loss_launch(d, n, target, weight, loss_slot, term_slot, grad_logit, (hipStream_t)stream);
}

int mcvc_adam_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long long n, float lr, float beta1, float beta2,
                   float eps, int step, float grad_scale, void* stream)
{
    return mcvc_adam_launch(p, const_cast<float*>(g), nullptr, 0, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, grad_scale, (hipStream_t)stream);
}

int mcvc_adam_step2(float* p, float* g, float* g2, int zero_grads, float* exp_avg, float* exp_avg_sq, long long n, float lr, float beta1, float beta2,
                    float eps, int step, float grad_scale, void* stream)
{
    return mcvc_adam_launch(p, g, g2, zero_grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, grad_scale, (hipStream_t)stream);
}

int mcvc_draw_batch(const float* bank_A, const int* offs_A, int n_A, long long frames_A, const float* bank_B, const int* offs_B, int n_B,
                    long long frames_B, int B, int T, int max_mask_len, unsigned long long seed, unsigned long long step,
                    float* real_A, float* mask_A, float* real_B, float* mask_B, int* draws, void* stream)
{
    if (!bank_A || !offs_A || !bank_B || !offs_B || n_A < 1 || n_B < 1 || !real_A || !mask_A || !real_B || !mask_B) return MCVC_ERR_INVALID;
    DrawArgs a{};
    a.bank[0] = bank_A; a.bank[1] = bank_B; a.offs[0] = offs_A; a.offs[1] = offs_B; a.ld[0] = frames_A; a.ld[1] = frames_B;
    a.n[0] = n_A; a.n[1] = n_B; a.B = B; a.T = T; a.max_mask_len = max_mask_len; a.seed = seed; a.step = step;
    a.real[0] = real_A; a.real[1] = real_B; a.mask[0] = mask_A; a.mask[1] = mask_B; a.draws = draws;
    return mcvc_draw_batch_launch(a, (hipStream_t)stream);
}

int mcvc_audio_frames(int n_samples) { return mcvc_audio_frames_of(n_samples); }

long long mcvc_audio_basis_floats(void) { return mcvc_audio_basis_floats_of(); }

int mcvc_audio_basis_init(float* basis)
{
    if (!basis || ((uintptr_t)basis & 3)) return MCVC_ERR_INVALID;
    mcvc_audio_basis_fill(basis);
    return MCVC_OK;
}

int mcvc_audio_plan(const int* sample_offs, int n_utts, int* frame_offs, int* tiles, int max_tiles, int* n_tiles)
{
    return mcvc_audio_plan_host(sample_offs, n_utts, frame_offs, tiles, max_tiles, n_tiles);
}

int mcvc_audio_log_mel(const float* wave, long long n_samples, const int* tiles, int n_tiles, const float* basis, float* out,
                       long long total_frames, void* stream)
{
    return mcvc_audio_log_mel_launch(wave, n_samples, tiles, n_tiles, basis, out, total_frames, (hipStream_t)stream);
}

// ---- MelGAN decoder (vocoder_kernels.hip) ----
int mcvc_voc_out_samples(int T) { return T < MCVC_VOC_MIN_FRAMES || T > (1 << 20) ? 0 : MCVC_VOC_HOP * T; }

int mcvc_voc_launches(void) { return MCVC_VOC_NLAUNCH; }

long long mcvc_voc_packed_floats(void) { return mcvc_voc_packed_floats_of(); }

int mcvc_voc_pack(const float* const* host_table, float* packed_host) { return mcvc_voc_pack_host(host_table, packed_host); }

long long mcvc_voc_workspace_floats(int B, int T) { return mcvc_voc_workspace_floats_of(B, T); }

int mcvc_voc_decode(const float* packed, const float* mel, float* out, float* workspace, long long workspace_floats, int B, int T, void* stream)
{
    return mcvc_voc_decode_launch(packed, mel, out, workspace, workspace_floats, B, T, (hipStream_t)stream);
}

long long mcvc_voc_layer_packed_floats(int kind, int Cin, int Cout, int k, int r) { return mcvc_voc_layer_packed_floats_of(kind, Cin, Cout, k, r); }

int mcvc_voc_layer_pack(int kind, const float* w0, const float* b0, const float* w1, const float* b1, float* packed_host, int Cin, int Cout, int k, int r)
{
    return mcvc_voc_layer_pack_host(kind, w0, b0, w1, b1, packed_host, Cin, Cout, k, r);
}

int mcvc_voc_layer(int kind, const float* packed, const float* x0, const float* x1, float* y, int B, int Cin, int Cout, int L, int k, int dilation, int r,
                   int act_in, void* stream)
{
    return mcvc_voc_layer_launch(kind, packed, x0, x1, y, B, Cin, Cout, L, k, dilation, r, act_in, (hipStream_t)stream);
}

// ---- Griffin-Lim decoder (griffinlim_kernels.hip) ----
int mcvc_gl_out_samples(int T) { return mcvc_gl_out_samples_of(T); }

int mcvc_gl_launches(int n_iter) { return mcvc_gl_launches_of(n_iter); }

long long mcvc_gl_tables_floats(void) { return mcvc_gl_tables_floats_of(); }

int mcvc_gl_tables_init(const float* host_pinv, float* host_out)
{
    if (!host_pinv || !host_out || ((uintptr_t)host_pinv & 3) || ((uintptr_t)host_out & 3)) return MCVC_ERR_INVALID;
    mcvc_gl_tables_fill(host_pinv, host_out);
    return MCVC_OK;
}

long long mcvc_gl_workspace_floats(int B, int T) { return mcvc_gl_workspace_floats_of(B, T); }

int mcvc_gl_decode(const float* in, int in_kind, const float* angles0, const float* tables, float* out, float* workspace,
                   long long workspace_floats, int B, int T, int n_iter, float momentum, void* stream)
{
    return mcvc_gl_decode_launch(in, in_kind, angles0, tables, out, workspace, workspace_floats, B, T, n_iter, momentum, (hipStream_t)stream);
}

// ---- mel inversion by non-negative least squares (melinv_kernels.hip) ----
int mcvc_melinv_max_iter(void) { return MCVC_MELINV_MAX_ITER; }

long long mcvc_melinv_tables_floats(void) { return mcvc_melinv_tables_floats_of(); }

int mcvc_melinv_tables_init(const float* host_basis, const float* host_pinv, double lambda, float* host_out)
{
    if (!host_basis || !host_pinv || !host_out || (((uintptr_t)host_basis | (uintptr_t)host_pinv | (uintptr_t)host_out) & 3)) return MCVC_ERR_INVALID;
    return mcvc_melinv_tables_fill(host_basis, host_pinv, lambda, host_out);
}

int mcvc_melinv_solve(const float* logmel, const float* tables, float* mag_out, int B, int T, int n_iter, void* stream)
{
    return mcvc_melinv_solve_launch(logmel, tables, mag_out, B, T, n_iter, (hipStream_t)stream);
}

// ---- objective evaluation: mel-cepstra and batched DTW (dtw_kernels.hip) ----
int mcvc_dtw_max_frames(void) { return MCVC_DTW_MAX_FRAMES; }

int mcvc_dtw_launches(int want_path) { return want_path ? 2 : 1; }

int mcvc_cep_basis_init(int n_cep, float* basis_host)
{
    if (!basis_host || ((uintptr_t)basis_host & 3)) return MCVC_ERR_INVALID;
    return mcvc_cep_basis_fill(n_cep, basis_host);
}

int mcvc_cep_project(const float* mel, long long n_frames, const float* basis, int n_cep, float* out, void* stream)
{
    return mcvc_cep_project_launch(mel, n_frames, basis, n_cep, out, (hipStream_t)stream);
}

int mcvc_dtw_plan(const int* x_offs, const int* y_offs, int n_pairs, int want_path, long long* table, long long* ws_bytes, long long* path_rows)
{
    return mcvc_dtw_plan_host(x_offs, y_offs, n_pairs, want_path, table, ws_bytes, path_rows);
}

int mcvc_dtw_run(const float* x, long long x_frames, const float* y, long long y_frames, int K, float scale, const int* x_offs, const int* y_offs,
                 const long long* table, int n_pairs, float* cost, int* length, int* path, void* workspace, long long workspace_bytes, void* stream)
{
    return mcvc_dtw_run_launch(x, x_frames, y, y_frames, K, scale, x_offs, y_offs, table, n_pairs, cost, length, path, workspace, workspace_bytes,
                               (hipStream_t)stream);
}

// ---- pitch tracking: YIN F0 contours and F0 statistics along DTW paths (f0_kernels.hip) ----
int mcvc_f0_max_lag(void) { return MCVC_F0_MAX_LAG; }

int mcvc_f0_launches(int want_cmnd) { (void)want_cmnd; return 1; }

int mcvc_f0_track(const float* wave, long long n_samples, const int* tiles, int n_tiles, int tau_min, int tau_max, float threshold, float* f0,
                  float* aperiodicity, float* cmnd, long long total_frames, void* stream)
{
    return mcvc_f0_track_launch(wave, n_samples, tiles, n_tiles, tau_min, tau_max, threshold, f0, aperiodicity, cmnd, total_frames, (hipStream_t)stream);
}

int mcvc_f0_stats(const float* fx, long long x_frames, const float* fy, long long y_frames, const int* path, const long long* pairs, int n_pairs,
                  int* counts, float* sums, void* stream)
{
    return mcvc_f0_stats_launch(fx, x_frames, fy, y_frames, path, pairs, n_pairs, counts, sums, (hipStream_t)stream);
}

// ---- non-parallel evaluation: modulation spectra, global variance and the distance between two sets (ms_kernels.hip) ----
int mcvc_ms_max_fft(void) { return MCVC_MS_MAX_FFT; }

int mcvc_ms_launches(void) { return MCVC_MS_LAUNCHES; }

int mcvc_ms_table_init(int n_fft, float* table_host)
{
    if (!table_host || ((uintptr_t)table_host & 3)) return MCVC_ERR_INVALID;
    return mcvc_ms_table_fill(n_fft, table_host);
}

int mcvc_ms_power(const float* cep, long long n_frames, int K, const int* offs_dev, int n_utts, const int* offs_host, int n_fft, const float* table,
                  float* power, float* mean, float* var, void* stream)
{
    return mcvc_ms_power_launch(cep, n_frames, K, offs_dev, n_utts, offs_host, n_fft, table, power, mean, var, (hipStream_t)stream);
}

int mcvc_ms_mean_log(const float* values, int n, long long R, float floor, float* out, void* stream)
{
    return mcvc_ms_mean_log_launch(values, n, R, floor, out, (hipStream_t)stream);
}

int mcvc_ms_distance(const float* a, const float* b, int K, int n_bins, int n_used, float* per_dim, float* total, void* stream)
{
    return mcvc_ms_distance_launch(a, b, K, n_bins, n_used, per_dim, total, (hipStream_t)stream);
}

// ---- sample-rate conversion: polyphase Kaiser filter on a bank of utterances (resample_kernels.hip) ----
int mcvc_resample_max_factor(void) { return MCVC_RESAMPLE_MAX_FACTOR; }

int mcvc_resample_tile_samples(void) { return MCVC_RESAMPLE_TILE; }

long long mcvc_resample_out_samples(long long n_in, int up, int down) { return mcvc_resample_out_samples_of(n_in, up, down); }

long long mcvc_resample_table_floats(int up, int down) { return mcvc_resample_table_floats_of(up, down); }

int mcvc_resample_pack(const float* h_host, int n_taps, int up, int down, float* table_host)
{
    return mcvc_resample_pack_host(h_host, n_taps, up, down, table_host);
}

int mcvc_resample_plan(const int* in_offs, int n_utts, int up, int down, int* out_offs, int* tiles, int max_tiles, int* n_tiles)
{
    return mcvc_resample_plan_host(in_offs, n_utts, up, down, out_offs, tiles, max_tiles, n_tiles);
}

int mcvc_resample_run(const float* x, long long n_in_total, const int* tiles, int n_tiles, const float* table, int up, int down, float* y,
                      long long n_out_total, void* stream)
{
    return mcvc_resample_run_launch(x, n_in_total, tiles, n_tiles, table, up, down, y, n_out_total, (hipStream_t)stream);
}

// ---- silence detection: frame energies of a bank of utterances (vad_kernels.hip) ----
int mcvc_vad_frame_length(void) { return MCVC_VAD_FRAME; }

int mcvc_vad_hop(void) { return MCVC_VAD_HOP; }

int mcvc_vad_tile_frames(void) { return MCVC_VAD_TILE_FRAMES; }

int mcvc_vad_launches(void) { return MCVC_VAD_LAUNCHES; }

long long mcvc_vad_frames(long long n) { return mcvc_vad_frames_of(n); }

int mcvc_vad_plan(const int* sample_offs, int n_utts, int* frame_offs, int* tiles, int max_tiles, int* n_tiles)
{
    return mcvc_vad_plan_host(sample_offs, n_utts, frame_offs, tiles, max_tiles, n_tiles);
}

int mcvc_vad_energy(const float* wave, long long n_samples, const int* tiles, int n_tiles, const int* frame_offs_dev, int n_utts, float* mse,
                    long long total_frames, float* ref, void* stream)
{
    return mcvc_vad_energy_launch(wave, n_samples, tiles, n_tiles, frame_offs_dev, n_utts, mse, total_frames, ref, (hipStream_t)stream);
}

int mcvc_audio_plan_segments(const int* starts, const int* lengths, int n_segs, int* frame_offs, int* tiles, int max_tiles, int* n_tiles)
{
    return mcvc_audio_plan_segments_host(starts, lengths, n_segs, frame_offs, tiles, max_tiles, n_tiles);
}

int mcvc_axpy(float* y, const float* x, float alpha, long long n, void* stream)
{
    return mcvc_axpy_launch(y, x, alpha, n, (hipStream_t)stream);
}

// ---- single-op entry points ----------------------------------------------------------------------------
static ConvSpec single_spec(int Cout, int Cin, int KH, int KW, int stride, int ph, int pw)
{
    ConvSpec c = mk(Cin, Cout, 1, KH, KW, stride, ph, pw, 0, 1, -1, -1, 1);
    long long cur = 0;
    spec_finalize(c, cur);
    c.off[PF_DCLS] = -1;               // (the single-op pack holds the merged matrix only)
    return c;
}

long long mcvc_conv2d_pack_floats(int Cout, int Cin, int KH, int KW)
{
    // stride-2 classes partition the taps (same rows in total) but each class carries its own zero pad row
    ConvSpec c = mk(Cin, Cout, 1, KH, KW, 1, 0, 0, 0, 1, -1, -1, 1);
    long long cur = 0;
    spec_finalize(c, cur);
    // stride 2 uses the merged parity layout: at most (KH+1)/2+1 x (KW+1)/2+1 taps x 4*Cin columns
    const long long merged = ((long long)c.dg_rows_co * ((KH + 1) / 2 + 1) * ((KW + 1) / 2 + 1) + 1) * round_up_i(4 * Cin, 32);
    return cur + merged + 4LL * c.cin_pk + 64;
}

int mcvc_conv2d_forward(const float* x, const float* w, const float* bias, float* y, float* wpack, float* slabs, int max_slabs,
                        int N, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad_h, int pad_w, int pixel_shuffle, void* stream)
{
    if (stride != 1 && stride != 2) return MCVC_ERR_INVALID;
    const ConvSpec c = single_spec(Cout, Cin, KH, KW, stride, pad_h, pad_w);
    Exec ex{}; ex.s = (hipStream_t)stream;
    ex.fail(mcvc_pack_fwd_launch(w, wpack + c.off[PF_FWD], Cout, Cin * KH * KW, c.cout_pk, 0, ex.s));
    if (bias) ex.fail(mcvc_copy_launch(bias, wpack + c.off[PF_BIAS], Cout, ex.s));
    const int OH = conv_out(H, KH, stride, pad_h), OW = conv_out(W, KW, stride, pad_w);
    const long long y_total = (long long)N * Cout * OH * OW;
    ex.slabs = slabs; ex.slab_cap = slabs ? (long long)(max_slabs - 1) * y_total : 0; ex.max_split = max_slabs > 0 ? max_slabs : 1;
    int ns = 1;
    const Tensor yv = pixel_shuffle ? nchw(y, N, Cout / 4, 2 * OH, 2 * OW) : nchw(y, N, Cout, OH, OW);
    ConvProblem p{Cin, H, W, Cout, OH, OW, KH, KW, stride, pad_h, pad_w};
    ConvIO io = conv_io(nchw(x, N, Cin, H, W), yv);
    io.shuffle = pixel_shuffle;
    int want = (slabs && max_slabs > 1) ? mcvc_conv_plan_nsplit(p, N, 1) : 1;
    if (want > max_slabs) want = max_slabs;
    run_conv(ex, p, N, io, y_total, wpack + c.off[PF_FWD], c.w_rows, c.cout_pk, bias ? wpack + c.off[PF_BIAS] : nullptr, 0, want, &ns);
    sum_slabs(ex, flat(y, y_total), ns);
    return ex.err;
}

int mcvc_conv2d_dgrad(const float* dy, const float* w, float* dx, float* wpack, float* slabs, int max_slabs, int N, int Cin, int H, int W,
                      int Cout, int KH, int KW, int stride, int pad_h, int pad_w, void* stream)
{
    if (stride != 1 && stride != 2) return MCVC_ERR_INVALID;
    const ConvSpec c = single_spec(Cout, Cin, KH, KW, stride, pad_h, pad_w);
    Exec ex{}; ex.s = (hipStream_t)stream;
    ex.fail(mcvc_pack_dgrad_launch(w, wpack + c.off[PF_DGRAD], dgrad_args(c, 0), Cout, ex.s));
    const int OH = conv_out(H, KH, stride, pad_h), OW = conv_out(W, KW, stride, pad_w);
    const long long dx_total = (long long)N * Cin * H * W;
    ex.slabs = slabs; ex.slab_cap = slabs ? (long long)(max_slabs - 1) * dx_total : 0; ex.max_split = max_slabs > 0 ? max_slabs : 1;
    int ns = 1;
    // positions of dx never written by any parity class do not exist: classes tile the whole input grid
    conv_dgrad(ex, c, wpack, nchw(dy, N, Cout, OH, OW), nchw(dx, N, Cin, H, W), 0, (slabs && max_slabs > 1) ? 1 : 0, &ns);
    if (ns > max_slabs && !ex.err) return MCVC_ERR_WORKSPACE;
    sum_slabs(ex, flat(dx, dx_total), ns);
    return ex.err;
}

long long mcvc_conv2d_wgrad_slab_floats(int N, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad_h, int pad_w)
{
    const int OH = conv_out(H, KH, stride, pad_h), OW = conv_out(W, KW, stride, pad_w);
    ConvProblem p{Cin, H, W, Cout, OH, OW, KH, KW, stride, pad_h, pad_w};
    return mcvc_wgrad_plan_slab_floats(p, N);
}

int mcvc_conv2d_wgrad(const float* x, const float* dy, float* dw, float* slabs, long long slab_floats, int N, int Cin, int H, int W, int Cout,
                      int KH, int KW, int stride, int pad_h, int pad_w, void* stream)
{
    const int OH = conv_out(H, KH, stride, pad_h), OW = conv_out(W, KW, stride, pad_w);
    ConvProblem p{Cin, H, W, Cout, OH, OW, KH, KW, stride, pad_h, pad_w};
    WgradIO io{x, (long long)Cin * H * W, (long long)H * W, W, dy, (long long)Cout * OH * OW, (long long)OH * OW, OW};
    // (the same special cases the network planner takes, conv_wgrad: dw accumulates, the caller passes zeros)
    if (Cout == 1 && mcvc_wgrad_cout1_applies(p)) return mcvc_wgrad_cout1_launch(p, N, io, dw, (hipStream_t)stream);
    if (mcvc_wgrad_cin2_applies(p, io)) return mcvc_wgrad_cin2_launch(p, N, io, dw, (hipStream_t)stream);
    return mcvc_wgrad_launch(p, N, io, dw, slabs, slab_floats, (hipStream_t)stream);
}

// ---- one convolution LAYER of the path, op by op, through the planner the networks use (conv_fwd / conv_dgrad / conv_wgrad) ----------
// SURVEY.md section 8(b) names single-op entries for the kernels that are hot at the trainer's shapes; the Winograd and staged-GEMM forms
// live inside the planner (their weight sets are job kinds of the whole-network pack), so the op-level ABI is the planner on ONE layer.
namespace {
struct LayerCtx { ConvSpec c; long long packed_floats; };
static LayerCtx layer_ctx(int Cin, int Cout, int nbr, int KH, int KW, int stride, int ph, int pw)
{
    LayerCtx l{};
    l.c = mk(Cin, Cout, nbr, KH, KW, stride, ph, pw, 0, 1, nbr == 2 ? 2 : -1, nbr == 2 ? 3 : -1, 1);
    long long cur = 0;
    spec_finalize(l.c, cur);
    l.packed_floats = cur + 64;
    return l;
}
struct LayerScratch { long long wv, wm, wv2, wm2, wino_floats, wu, wu_floats, tail; };
static LayerScratch layer_scratch(const ConvSpec& c, int N, int H, int W)
{
    LayerScratch q{};
    long long cur = 0;
    auto take = [&](long long n) { const long long o = cur; cur += (n + 3) & ~3LL; return o; };
    const long long tiles2 = (((long long)N * ((H + 1) / 2) * ((W + 1) / 2) + 63) & ~63LL) + 64;
    const long long chan = std::max<long long>(std::max(4LL * c.Cin, (long long)c.cout_tot), 64);
    q.wino_floats = 36LL * chan * tiles2;
    q.wv = take(q.wino_floats); q.wm = take(q.wino_floats); q.wv2 = take(q.wino_floats); q.wm2 = take(q.wino_floats);
    q.wu_floats = 64LL * c.cout_tot * 4 * c.Cin;
    q.wu = take(q.wu_floats);
    q.tail = cur;
    return q;
}
static Needs layer_needs(const ConvSpec& c, int N, int H, int W, int scheme)
{
    Exec ex{}; ex.dry = true; ex.force_scheme = scheme;
    const LayerScratch q = layer_scratch(c, N, H, W);
    ex.wv = ex.wm = ex.wv2 = ex.wm2 = ex.wu = reinterpret_cast<float*>(16);      // (non-null: the dry run only looks at capacities)
    ex.wino_cap = q.wino_floats; ex.wu_cap = q.wu_floats;
    const int OH = conv_out(H, c.KH, c.stride, c.ph), OW = conv_out(W, c.KW, c.stride, c.pw);
    int ns = 1;
    float* const none = nullptr;
    const Tensor x = nchw(none, N, c.Cin, H, W), y = nchw(none, N, c.cout_tot, OH, OW);
    conv_fwd(ex, c, nullptr, x, y, 0, 1, &ns);
    conv_dgrad(ex, c, nullptr, y, x, 0, 1, &ns);
    conv_wgrad(ex, c, nullptr, x, y);
    if (igemm_applies(c, H, W)) {
        const Tensor xs = phase_split(none, N, c.Cin, H, W);
        conv_fwd_igemm(ex, c, nullptr, xs, y, 1, &ns);
        conv_dgrad_igemm(ex, c, nullptr, padded_dy(none, N, c.cout_tot, OH, OW), x, 0, 1, &ns);
        conv_wgrad(ex, c, nullptr, xs, y);             // (the implicit weight gradient's K-split slabs)
    }
    return Needs{(ex.slab_need + 3) & ~3LL, (ex.wslab_need + 3) & ~3LL, (ex.sg_need + 3) & ~3LL, (ex.sgw_need + 3) & ~3LL};
}
struct SchemeGuard {            // scheme 3: no Winograd; 4: neither Winograd nor staged GEMM (thread-local planner switches)
    int w, g, u;
    explicit SchemeGuard(int scheme) : w(t_no_wino), g(t_no_sgemm), u(t_user_operands) { if (scheme >= 3) t_no_wino = 1; if (scheme == 4) t_no_sgemm = 1; t_user_operands = 1; }
    ~SchemeGuard() { t_no_wino = w; t_no_sgemm = g; t_user_operands = u; }
};
static Exec layer_exec(const ConvSpec& c, int N, int H, int W, int scheme, float* scratch, long long scratch_floats, void* stream, int* err)
{
    const LayerScratch q = layer_scratch(c, N, H, W);
    const Needs nd = layer_needs(c, N, H, W, scheme);
    Exec ex = make_exec(stream, nullptr, scratch, scratch_floats, q.tail, nd);
    if (ex.wslab_cap < 0) { *err = MCVC_ERR_WORKSPACE; return ex; }
    ex.wv = scratch + q.wv; ex.wm = scratch + q.wm; ex.wv2 = scratch + q.wv2; ex.wm2 = scratch + q.wm2; ex.wino_cap = q.wino_floats;
    ex.wu = scratch + q.wu; ex.wu_cap = q.wu_floats;
    ex.force_scheme = scheme;
    return ex;
}
}  // namespace

long long mcvc_layer_packed_floats(int Cin, int Cout, int branches, int KH, int KW, int stride, int pad_h, int pad_w)
{
    if (branches < 1 || branches > 2 || (stride != 1 && stride != 2)) return -1;
    return layer_ctx(Cin, Cout, branches, KH, KW, stride, pad_h, pad_w).packed_floats;
}

long long mcvc_layer_scratch_floats(int N, int H, int W, int Cin, int Cout, int branches, int KH, int KW, int stride, int pad_h, int pad_w)
{
    if (branches < 1 || branches > 2 || (stride != 1 && stride != 2) || N < 1) return -1;
    const LayerCtx l = layer_ctx(Cin, Cout, branches, KH, KW, stride, pad_h, pad_w);
    long long worst = 0;
    for (int scheme = 0; scheme <= 4; ++scheme) {
        SchemeGuard sg(scheme);
        const Needs nd = layer_needs(l.c, N, H, W, scheme);
        const long long need = nd.slab + nd.wslab + nd.sg + nd.sgw;
        if (need > worst) worst = need;
    }
    ConvProblem p{Cin, H, W, Cout, conv_out(H, KH, stride, pad_h), conv_out(W, KW, stride, pad_w), KH, KW, stride, pad_h, pad_w};
    return layer_scratch(l.c, N, H, W).tail + worst + mcvc_wgrad_plan_slab_floats(p, N) + 1024;
}

int mcvc_layer_pack(const float* w0, const float* b0, const float* w1, const float* b1, float* packed, int Cin, int Cout, int branches,
                    int KH, int KW, int stride, int pad_h, int pad_w, void* stream)
{
    if (!w0 || !b0 || !packed || branches < 1 || branches > 2 || (branches == 2 && (!w1 || !b1))) return MCVC_ERR_INVALID;
    const LayerCtx l = layer_ctx(Cin, Cout, branches, KH, KW, stride, pad_h, pad_w);
    // the job table of this layer alone (cached per device and layer shape like the networks' tables)
    PackPlan k;
    k.net = 2; k.shape = {Cin, Cout, branches, KH, KW, stride, pad_h, pad_w};
    k.add(l.c, kAllForms);
    const ConvSpec* spec = &l.c;
    int err = 0;
    const DevPackTable* t = dev_pack_table(k, &spec, &err);
    if (!t) return err ? err : MCVC_ERR_INVALID;
    const float* params[4] = {w0, b0, w1, b1};
    return pack_net(t, params, packed, (hipStream_t)stream);
}

int mcvc_layer_forward(const float* x, const float* packed, const float* w0, const float* w1, float* y, float* scratch, long long scratch_floats,
                       int N, int H, int W, int Cin, int Cout, int branches, int KH, int KW, int stride, int pad_h, int pad_w, int scheme,
                       int pixel_shuffle, void* stream)
{
    if (!x || !packed || !y || !scratch || scheme < 0 || scheme > 5 || branches < 1 || branches > 2 || (stride != 1 && stride != 2)) return MCVC_ERR_INVALID;
    const LayerCtx l = layer_ctx(Cin, Cout, branches, KH, KW, stride, pad_h, pad_w);
    if ((scheme == 1 || scheme == 2) && !(l.c.wino || l.c.wino3)) return MCVC_ERR_INVALID;       // no Winograd form of this layer shape
    if (scheme == 5) {          // implicit GEMM (sgemm.h): the dense input is converted to the phase-split padded layout the networks' producers write
        if (!igemm_applies(l.c, H, W) || pixel_shuffle) return MCVC_ERR_INVALID;
        int err5 = 0;
        Exec ex5 = layer_exec(l.c, N, H, W, 0, scratch, scratch_floats, stream, &err5);
        if (err5) return err5;
        if ((long long)N * mcvc_xs_floats(Cin, H, W) > ex5.wino_cap) return MCVC_ERR_WORKSPACE;
        ex5.fail(mcvc_xs_from_dense_launch(x, ex5.wv, N, Cin, H, W, ex5.s));
        const Tensor yv5 = nchw(y, N, l.c.cout_tot, H / 2, W / 2);
        int ns5 = 1;
        conv_fwd_igemm(ex5, l.c, packed, phase_split(ex5.wv, N, Cin, H, W), yv5, 1, &ns5);
        sum_slabs(ex5, flat(y, yv5.dense()), ns5);
        return ex5.err;
    }
    SchemeGuard sg(scheme);
    int err = 0;
    Exec ex = layer_exec(l.c, N, H, W, scheme, scratch, scratch_floats, stream, &err);
    if (err) return err;
    const float* params[4] = {w0, nullptr, w1, nullptr};
    ex.params = params;
    const int OH = conv_out(H, KH, stride, pad_h), OW = conv_out(W, KW, stride, pad_w);
    const Tensor yv = pixel_shuffle ? nchw(y, N, l.c.cout_tot / 4, 2 * OH, 2 * OW) : nchw(y, N, l.c.cout_tot, OH, OW);
    int ns = 1;
    conv_fwd(ex, l.c, packed, nchw(x, N, Cin, H, W), yv, pixel_shuffle, 1, &ns);
    sum_slabs(ex, flat(y, yv.dense()), ns);
    return ex.err;
}

int mcvc_layer_dgrad(const float* dy, const float* packed, const float* w0, const float* w1, float* dx, float* scratch, long long scratch_floats,
                     int N, int H, int W, int Cin, int Cout, int branches, int KH, int KW, int stride, int pad_h, int pad_w, int scheme, void* stream)
{
    if (!dy || !packed || !dx || !scratch || scheme < 0 || scheme > 5 || branches < 1 || branches > 2 || (stride != 1 && stride != 2)) return MCVC_ERR_INVALID;
    const LayerCtx l = layer_ctx(Cin, Cout, branches, KH, KW, stride, pad_h, pad_w);
    const Tensor dxv = nchw(dx, N, Cin, H, W);
    if (scheme == 5) {          // implicit GEMM: the four parity classes scattered straight into dx; the dense dY is padded first (the networks' norm_bwd writes it padded)
        if (!igemm_applies(l.c, H, W)) return MCVC_ERR_INVALID;
        int err5 = 0;
        Exec ex5 = layer_exec(l.c, N, H, W, 0, scratch, scratch_floats, stream, &err5);
        if (err5) return err5;
        const int OH5 = H / 2, OW5 = W / 2;
        if ((long long)N * l.c.cout_tot * mcvc_dyp_plane(OH5, OW5) > ex5.wino_cap) return MCVC_ERR_WORKSPACE;
        ex5.fail(mcvc_dyp_from_dense_launch(dy, ex5.wm, N, l.c.cout_tot, OH5, OW5, ex5.s));
        int ns5 = 1;
        conv_dgrad_igemm(ex5, l.c, packed, padded_dy(ex5.wm, N, l.c.cout_tot, OH5, OW5), dxv, 0, 1, &ns5);
        sum_slabs(ex5, flat(dx, dxv.dense()), ns5);
        return ex5.err;
    }
    SchemeGuard sg(scheme);
    int err = 0;
    Exec ex = layer_exec(l.c, N, H, W, scheme, scratch, scratch_floats, stream, &err);
    if (err) return err;
    const float* params[4] = {w0, nullptr, w1, nullptr};
    ex.params = (w0 && (branches == 1 || w1)) ? params : nullptr;         // (the staged-GEMM data gradient multiplies the OIHW tensors themselves)
    const int OH = conv_out(H, KH, stride, pad_h), OW = conv_out(W, KW, stride, pad_w);
    int ns = 1;
    conv_dgrad(ex, l.c, packed, nchw(dy, N, l.c.cout_tot, OH, OW), dxv, 0, 1, &ns);
    sum_slabs(ex, flat(dx, dxv.dense()), ns);
    return ex.err;
}

int mcvc_layer_wgrad(const float* x, const float* dy, float* dw0, float* dw1, float* scratch, long long scratch_floats, int N, int H, int W,
                     int Cin, int Cout, int branches, int KH, int KW, int stride, int pad_h, int pad_w, int scheme, void* stream)
{
    return mcvc_layer_wgrad_flags(x, dy, dw0, dw1, scratch, scratch_floats, N, H, W, Cin, Cout, branches, KH, KW, stride, pad_h, pad_w, scheme, 0, stream);
}

// ... with the backward passes' flags: MCVC_BWD_STORE_GRADS runs conv_wgrad in store mode on this ONE layer (a covered layer's gradient is
// stored, an uncovered one's accumulated into: the planner's rule, reachable per layer for the tests)
int mcvc_layer_wgrad_flags(const float* x, const float* dy, float* dw0, float* dw1, float* scratch, long long scratch_floats, int N, int H, int W,
                           int Cin, int Cout, int branches, int KH, int KW, int stride, int pad_h, int pad_w, int scheme, int flags, void* stream)
{
    if (flags & ~MCVC_BWD_STORE_GRADS) return MCVC_ERR_INVALID;
    const int store = (flags & MCVC_BWD_STORE_GRADS) ? 1 : 0;
    if (!x || !dy || !dw0 || !scratch || scheme < 0 || scheme > 5 || branches < 1 || branches > 2 || (branches == 2 && !dw1)) return MCVC_ERR_INVALID;
    const LayerCtx l = layer_ctx(Cin, Cout, branches, KH, KW, stride, pad_h, pad_w);
    const int OH = conv_out(H, KH, stride, pad_h), OW = conv_out(W, KW, stride, pad_w);
    if (scheme == 5) {          // implicit weight gradient (wgemm_kernels.hip): the dense input is converted to the phase-split padded layout first
        if (!igemm_applies(l.c, H, W)) return MCVC_ERR_INVALID;
        int err5 = 0;
        Exec ex5 = layer_exec(l.c, N, H, W, 0, scratch, scratch_floats, stream, &err5);
        if (err5) return err5;
        if ((long long)N * mcvc_xs_floats(Cin, H, W) > ex5.wino_cap) return MCVC_ERR_WORKSPACE;
        ex5.fail(mcvc_xs_from_dense_launch(x, ex5.wv, N, Cin, H, W, ex5.s));
        float* grads5[4] = {dw0, nullptr, dw1, nullptr};
        ex5.store_grads = store;
        conv_wgrad(ex5, l.c, grads5, phase_split(ex5.wv, N, Cin, H, W), nchw(dy, N, l.c.cout_tot, OH, OW));
        return ex5.err;
    }
    SchemeGuard sg(scheme);
    int err = 0;
    Exec ex = layer_exec(l.c, N, H, W, scheme, scratch, scratch_floats, stream, &err);
    if (err) return err;
    float* grads[4] = {dw0, nullptr, dw1, nullptr};
    ex.store_grads = store;
    conv_wgrad(ex, l.c, grads, nchw(x, N, Cin, H, W), nchw(dy, N, l.c.cout_tot, OH, OW));
    return ex.err;
}

// The fused backward of one 1-D trunk layer (resblock1d_bwd / gemm1x1_in_bwd; reference model.py:47-76 under autograd):
// InstanceNorm (+ gated GLU) backward of dy recomputed inside the transposed-convolution launch (trunk_layer_kernel<.., PRE>), d(gamma), d(beta)
// accumulated, dconv = the gradient w.r.t. the conv output stored, dx += the data gradient, and (x_in != NULL) the weight gradients by the
// batched small-K kernel.  Trunk layout [C][B][T4] for every tensor; gate pointers NULL = plain InstanceNorm (no GLU).
int mcvc_trunk_layer_backward(const float* dy, const float* conv_out, const float* stats, const float* gamma, const float* beta,
                              const float* gamma_gate, const float* beta_gate, const float* w, const float* w_gate, const float* x_in,
                              float* dx, float* dconv, float* dgamma, float* dbeta, float* dgamma_gate, float* dbeta_gate, float* dw, float* dw_gate,
                              float* wpack, int B, int Cin, int T4, int Cout, int KW, void* stream)
{
    if (!dy || !conv_out || !stats || !gamma || !beta || !w || !dx || !dconv || !wpack || (KW != 1 && KW != 3)) return MCVC_ERR_INVALID;
    const bool glu = w_gate != nullptr;
    if (glu && (!gamma_gate || !beta_gate)) return MCVC_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int Cx = glu ? 2 * Cout : Cout;
    int rc = mcvc_pack_trunk_t_launch(w, wpack, Cout, Cin, KW, Cx * KW, 0, s);
    if (!rc && glu) rc = mcvc_pack_trunk_t_launch(w_gate, wpack, Cout, Cin, KW, Cx * KW, Cout, s);
    if (rc) return rc;
    const int ks = trunk_pick_ksplit(Cx, KW, Cin, B, T4, 0);
    if (ks < 1) return MCVC_ERR_INVALID;
    TrunkArgs a{};
    a.a0 = wpack;
    a.x = dy; a.x_sc = (long long)B * T4; a.x_sb = T4;
    a.Cin = Cx; a.KW = KW; a.K = Cx * KW; a.M = Cin; a.Mtot = Cin; a.B = B; a.T4 = T4; a.N = B * T4;
    a.conv_out = dx; a.c_sc = (long long)B * T4; a.c_sb = T4; a.accumulate = 1; a.mode = TRUNK_PLAIN;
    a.pre = glu ? 2 : 1; a.pre_C = Cout; a.pre_x = conv_out; a.pre_stats = stats;
    a.pre_gamma0 = gamma; a.pre_beta0 = beta; a.pre_gamma1 = gamma_gate; a.pre_beta1 = beta_gate;
    a.pre_out = dconv; a.pre_dgamma0 = dgamma; a.pre_dbeta0 = dbeta; a.pre_dgamma1 = dgamma_gate; a.pre_dbeta1 = dbeta_gate;
    if (ks > 1 && mcvc_deterministic()) {          // no atomics into dx: the K slices one launch after the other (this entry has no slab workspace)
        a.ky_n = ks;
        for (a.ky0 = 0; a.ky0 < ks && !rc; ++a.ky0) rc = mcvc_trunk_launch(a, ks, s);
    } else rc = mcvc_trunk_launch(a, ks, s);
    if (rc || !x_in || !dw) return rc;
    if (KW != 3 || !mcvc_wgrad_smallk_batch_applies(B, T4)) return MCVC_ERR_INVALID;
    SmallKJob jobs[2];
    int nj = 0;
    jobs[nj++] = SmallKJob{x_in, dconv, dw, Cin, Cout, 0, 0};
    if (glu && dw_gate) jobs[nj++] = SmallKJob{x_in, dconv + (long long)Cout * B * T4, dw_gate, Cin, Cout, 0, 0};
    return mcvc_wgrad_smallk_batch_launch(jobs, nj, B, T4, s);
}

int mcvc_instnorm_act_forward(float* x, const float* gamma, const float* beta, const float* gamma_gate, const float* beta_gate,
                              const float* residual, float* y, float* stats, int N, int C, int H, int W, int act, void* stream)
{
    Exec ex{}; ex.s = (hipStream_t)stream;
    NormP np{}; np.g[0] = gamma; np.b[0] = beta; np.g[1] = gamma_gate; np.b[1] = beta_gate;
    const int Cx = (act == ACT_GLU) ? 2 * C : C;
    norm_fwd(ex, nchw(x, N, Cx, H, W), 1, np, stats, nchw(y, N, C, H, W), residual, act);
    return ex.err;
}

int mcvc_instnorm_act_backward(const float* x, const float* gamma, const float* beta, const float* gamma_gate, const float* beta_gate,
                               const float* stats, float* dy, float* dx, float* dgamma, float* dbeta, float* dgamma_gate, float* dbeta_gate,
                               int N, int C, int H, int W, int act, void* stream)
{
    Exec ex{}; ex.s = (hipStream_t)stream;
    NormP np{}; np.g[0] = gamma; np.b[0] = beta; np.g[1] = gamma_gate; np.b[1] = beta_gate;
    np.dg[0] = dgamma; np.db[0] = dbeta; np.dg[1] = dgamma_gate; np.db[1] = dbeta_gate;
    const int Cx = (act == ACT_GLU) ? 2 * C : C;
    norm_bwd(ex, nchw(x, N, Cx, H, W), np, stats, nchw(dy, N, C, H, W), 1, nchw(dx, N, Cx, H, W), 0, act);
    return ex.err;
}

// fused 1-D trunk layer (small batch): conv1d(k = 1 or 3, pad (k-1)/2) + bias + InstanceNorm1d(affine) + {gated GLU | + residual | nothing}
int mcvc_trunk_layer_forward(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, const float* w_gate,
                             const float* bias_gate, const float* gamma_gate, const float* beta_gate, const float* residual, float* conv_out,
                             float* stats, float* y, int B, int Cin, int T4, int Cout, int KW, void* stream)
{
    if (!x || !w || !bias || !gamma || !beta || !conv_out || !stats || !y) return MCVC_ERR_INVALID;
    const int mode = w_gate ? TRUNK_IN_GLU : TRUNK_IN;
    if (!mcvc_trunk_applies(Cin, KW, Cout, B, T4, mode, 1)) return MCVC_ERR_INVALID;
    TrunkArgs a{};
    a.a0 = w; a.bias0 = bias; a.gamma0 = gamma; a.beta0 = beta;
    a.a1 = w_gate; a.bias1 = bias_gate; a.gamma1 = gamma_gate; a.beta1 = beta_gate;
    a.x = x; a.x_sc = (long long)B * T4; a.x_sb = T4;
    a.Cin = Cin; a.KW = KW; a.K = Cin * KW; a.M = Cout; a.Mtot = w_gate ? 2 * Cout : Cout; a.B = B; a.T4 = T4; a.N = B * T4;
    a.conv_out = conv_out; a.c_sc = (long long)B * T4; a.c_sb = T4;
    a.stats = stats; a.y = y; a.res = residual; a.y_sn = T4; a.y_sc = (long long)B * T4; a.eps = kInEps; a.mode = mode;
    return mcvc_trunk_launch(a, 1, (hipStream_t)stream);
}

// batched fp32 GEMM of the Winograd paths: C[x] = A[x]^T-major product, A K-major ([K][lda] rows of M), B [K][ldb], C [M][ldc]
int mcvc_batched_gemm(const float* a, const float* b, float* c, int nbatch, int M, int N, int K, int lda, int ldb, int ldc,
                      long long a_stride, long long b_stride, long long c_stride, void* stream)
{
    if (!a || !b || !c || nbatch < 1) return MCVC_ERR_INVALID;
    WinoGemmArgs ga{};
    ga.a = a; ga.a_xi = a_stride; ga.lda = lda; ga.b = b; ga.b_xi = b_stride; ga.ldb = ldb; ga.c = c; ga.c_xi = c_stride; ga.ldc = ldc;
    ga.M = M; ga.N = N; ga.K = K; ga.nxi = nbatch;
    return mcvc_wino_gemm_launch(ga, (hipStream_t)stream);
}

int mcvc_bias_grad(const float* dy, float* db, int N, int C, int P, void* stream)
{
    return mcvc_bias_grad_launch(dy, (long long)C * P, (long long)P, N, C, P, db, (hipStream_t)stream);
}

int mcvc_act_forward(float* x, float* y, int N, int C, int P, int act, void* stream)
{
    Exec ex{}; ex.s = (hipStream_t)stream;
    act_fwd(ex, nchw(x, N, act == ACT_GLU ? 2 * C : C, 1, P), 1, nchw(y, N, C, 1, P), act);
    return ex.err;
}

int mcvc_act_backward(const float* x, float* dy, float* dx, int N, int C, int P, int act, void* stream)
{
    Exec ex{}; ex.s = (hipStream_t)stream;
    const int Cx = act == ACT_GLU ? 2 * C : C;
    act_bwd(ex, nchw(x, N, Cx, 1, P), nchw(dy, N, C, 1, P), 1, nchw(dx, N, Cx, 1, P), act);
    return ex.err;
}

int mcvc_fif_input(const float* x, const float* mask, float* xin, int N, int P, void* stream)
{
    return mcvc_prep_input_launch(x, mask, xin, N, P, (hipStream_t)stream);
}

int mcvc_fif_input_grad(const float* dxin, const float* mask, float* dx, int N, int P, int accumulate, void* stream)
{
    return mcvc_mask_grad_launch(dxin, nullptr, 0, 1, mask, dx, N, P, 2, accumulate, (hipStream_t)stream);
}

}  // extern "C"
