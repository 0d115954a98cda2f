// The catalogue of packed weight forms: every derived copy of a convolution's weights that the kernels read is ONE row of kPackForms --
// what it is (job kind, reader side, which layers have it), where it lies (size, alignment, leading dimension, stride per transform
// point) and what refreshing it costs (grid, floats read / written).  The layout of a packed buffer (spec_finalize), the job tables of
// the re-pack and the fused update (add_spec_jobs) and the staleness records (net.hip) are all walks over these rows.
// Host-only planning code: nothing here calls the HIP runtime.
#pragma once
#include "pack.h"
#include "mcvc_common.h"
#include <vector>

enum PackForm {            // in the order a layer's jobs enter a table
    PF_FWD,                // K-major forward copy Wt[k][co] (+ zero pad row)
    PF_BIAS,
    PF_DGRAD,              // data-gradient copy: per class (stride 1) or the merged parity matrix (stride 2)
    PF_DCLS,               // exact per-class data-gradient copies of the 3x3 stride-2 layers (large batch)
    PF_TRUNK_T,            // KH == 1 convs: transposed + flipped [Cin][cout_tot*KW] copy for the fused small-batch trunk dgrad
    PF_IFWD,               // tap-major forward copy (implicit GEMM, sgemm.h; read row-major it is the data gradient's operand too)
    PF_W3D, PF_W3F,        // 5x5 stride-2 layers (downSample1/2): 16-point F(2x2,3x3) sets, data gradient / forward over the four input phases
    PF_W43D, PF_W43F,      // ... and their 36-point F(4x4,3x3) sets (wino43_kernels.hip)
    PF_W4F, PF_W4D,        // 5x5 stride-1 layers (upSample1/2): 64-point F(4x4,5x5) sets (wino4.h)
    PF_W2F, PF_W2D,        // ... and their 36-point F(2x2,5x5) sets
    kNumForms
};
constexpr unsigned kAllForms = (1u << kNumForms) - 1;
constexpr unsigned form_bit(PackForm f) { return 1u << f; }

struct ConvSpec {
    int Cin, Cout, nbr, KH, KW, stride, ph, pw;
    int wi[2], bi[2];
    int has_bias_grad;
    int index;                     // position of the layer in its network (op-level layers: 0): the staleness records are per layer
    // derived
    int cout_tot, cout_pk, cin_pad, w_rows, cin_pk, dg_rows_co;
    long long off[kNumForms];      // float offset of each form inside the packed buffer, -1: the layer has no such form
    int wino;                      // 5x5 stride-1 single-branch convs (upSample1/2): Winograd weight sets U[pts][K+1][ld], forward and data-gradient
    int wino3;                     // 5x5 stride-2 convs (downSample1/2): their merged 3x3 data-gradient (and the forward over the input phases) as Winograd
    int ncls;
    DgradClass cls[4];
    // stride 2: the four output-parity classes are ONE stride-1 conv with 4*Cin output channels (4*ci + 2*qh + qw) whose
    // taps are zero-padded to a common window; its PixelShuffle(2) store scatters straight into dX[ci][2a+qh][2b+qw]
    int merged, mg_kh, mg_kw, mg_pad_h, mg_pad_w, mg_ld;
    // 3x3 stride-2 convs (the discriminators') at large batch: the merged matrix multiplies 16 tap slots of which 9 are non-zero; with
    // enough pixels to fill the chip per launch the four parity classes run as four exact stride-1 convs instead (1.78x fewer MACs)
    DgradClass ucls[4];
    // 3x3 stride-2 padding-1 layers (the discriminators'): implicit-GEMM operands (sgemm.h) -- the forward copy with tap-major rows, which the
    // four parity classes of the data gradient read row-major
    int igemm; DgradClass icls[4];
};

enum PackSide { PACK_SIDE_FWD = 1, PACK_SIDE_BWD = 2 };      // which pass reads a form (the `sets` bits of mcvc_gen_pack_sets)
struct PackFormRow {
    PackKind kind;                            // what the pack kernels dispatch on
    int side;
    bool (*has)(const ConvSpec&);             // the layer has this form
    int pts;                                  // transform points (1: not a Winograd set)
    long long (*xi)(const ConvSpec&);         // floats per point, zero pad rows included: the form holds pts * xi floats
    bool align_before, align_after;           // round the cursor up to 4 floats in front of the form (when present) / behind it (always)
    int (*ld)(const ConvSpec&);               // leading dimension of its job (0: the job carries none)
    int (*gx)(const ConvSpec&); int (*gy)(const ConvSpec&);      // workgroup grid of its job, per branch
    int rd, wr;                               // floats read / written per filter (0: the filter's taps), the trace's byte accounting
};

namespace packforms {
typedef const ConvSpec& S;
inline long long dgrad_class_floats(S c, const DgradClass& k) { return ((long long)c.dg_rows_co * k.nth * k.ntw + 1) * c.cin_pk; }      // + zero pad row
inline long long per_class_floats(S c) { long long n = 0; for (int k = 0; k < c.ncls; ++k) n += dgrad_class_floats(c, c.cls[k]); return n; }
inline bool always(S) { return true; }
inline bool has_dcls(S c) { return c.stride == 2 && c.KH == 3 && c.KW == 3 && c.Cin >= 64; }
inline bool has_trunk_t(S c) { return c.KH == 1 && c.stride == 1; }
inline bool has_igemm(S c) { return c.igemm != 0; }
inline bool has_wino(S c) { return c.wino != 0; }
inline bool has_wino3(S c) { return c.wino3 != 0; }
inline long long fwd_floats(S c) { return (long long)(c.w_rows + 1) * c.cout_pk; }                  // + one all-zero pad row (DMA target for k >= K)
inline long long bias_floats(S c) { return c.cout_pk; }
inline long long dgrad_floats(S c) { return c.merged ? ((long long)c.dg_rows_co * c.mg_kh * c.mg_kw + 1) * c.mg_ld : per_class_floats(c); }
inline long long trunk_t_floats(S c) { return (long long)c.Cin * c.cout_tot * c.KW; }
inline long long ifwd_floats(S c) { return 9LL * c.Cin * c.cout_pk; }
inline long long xi_f5(S c) { return (long long)(c.cin_pad + 1) * c.cout_pk; }                      // rows ci (+ zero pad row), columns co
inline long long xi_d5(S c) { return (long long)(c.dg_rows_co + 1) * c.cin_pk; }                    // rows co, columns ci
inline long long xi_d3(S c) { return (long long)(c.dg_rows_co + 1) * c.mg_ld; }                     // U[pts][co (+1)][mg_ld]
inline long long xi_f3(S c) { return (long long)(4 * c.Cin + 1) * c.cout_pk; }                      // U[pts][4*Cin (+1)][cout_pk]
inline int ld_none(S) { return 0; }
inline int ld_cout(S c) { return c.cout_pk; }
inline int ld_cin(S c) { return c.cin_pk; }
inline int ld_mg(S c) { return c.mg_ld; }
inline int ld_trunk_t(S c) { return c.cout_tot * c.KW; }
inline int one(S) { return 1; }
inline int cout(S c) { return c.Cout; }
inline int cin(S c) { return c.Cin; }
inline int k_32(S c) { return cdiv_i(c.Cin * c.KH * c.KW, 32); }
inline int cin_32(S c) { return cdiv_i(c.Cin, 32); }
inline int cout_32(S c) { return cdiv_i(c.Cout, 32); }
inline int cin_256(S c) { return cdiv_i(c.Cin, 256); }
inline int cout_256(S c) { return cdiv_i(c.Cout, 256); }
}  // namespace packforms

static const PackFormRow kPackForms[kNumForms] = {
    //                kind           side           has                     pts  floats per point          align          ld                     grid                                    rd  wr
    /* PF_FWD     */ {PACK_FWD,      PACK_SIDE_FWD, packforms::always,      1,  packforms::fwd_floats,     false, false, packforms::ld_cout,    packforms::k_32,     packforms::cout_32, 0,  0},
    /* PF_BIAS    */ {PACK_COPY,     PACK_SIDE_FWD, packforms::always,      1,  packforms::bias_floats,    false, false, packforms::ld_none,    packforms::cout_256, packforms::one,     1,  1},
    /* PF_DGRAD   */ {PACK_DGRAD,    PACK_SIDE_BWD, packforms::always,      1,  packforms::dgrad_floats,   false, false, packforms::ld_none,    packforms::cin_32,   packforms::cout,    0,  0},
    /* PF_DCLS    */ {PACK_DGRAD,    PACK_SIDE_BWD, packforms::has_dcls,    1,  packforms::per_class_floats, true, false, packforms::ld_none,   packforms::cin_32,   packforms::cout,    0,  0},
    /* PF_TRUNK_T */ {PACK_TRUNK_T,  PACK_SIDE_BWD, packforms::has_trunk_t, 1,  packforms::trunk_t_floats, false, true,  packforms::ld_trunk_t, packforms::cin_32,   packforms::cout_32, 0,  0},
    /* PF_IFWD    */ {PACK_FWD_TAP,  PACK_SIDE_FWD, packforms::has_igemm,   1,  packforms::ifwd_floats,    true,  true,  packforms::ld_cout,    packforms::k_32,     packforms::cout_32, 0,  0},
    /* PF_W3D     */ {PACK_WINO3_D,  PACK_SIDE_BWD, packforms::has_wino3,   16, packforms::xi_d3,          false, true,  packforms::ld_mg,      packforms::cin_256,  packforms::cout,    25, 64},
    /* PF_W3F     */ {PACK_WINO3_F,  PACK_SIDE_FWD, packforms::has_wino3,   16, packforms::xi_f3,          false, true,  packforms::ld_cout,    packforms::cout_256, packforms::cin,     25, 64},
    /* PF_W43D    */ {PACK_WINO43_D, PACK_SIDE_BWD, packforms::has_wino3,   36, packforms::xi_d3,          false, true,  packforms::ld_mg,      packforms::cin_256,  packforms::cout,    25, 144},
    /* PF_W43F    */ {PACK_WINO43_F, PACK_SIDE_FWD, packforms::has_wino3,   36, packforms::xi_f3,          false, true,  packforms::ld_cout,    packforms::cout_256, packforms::cin,     25, 144},
    /* PF_W4F     */ {PACK_WINO4_F,  PACK_SIDE_FWD, packforms::has_wino,    64, packforms::xi_f5,          false, false, packforms::ld_cout,    packforms::cout_256, packforms::cin,     25, 64},
    /* PF_W4D     */ {PACK_WINO4_D,  PACK_SIDE_BWD, packforms::has_wino,    64, packforms::xi_d5,          false, true,  packforms::ld_cin,     packforms::cin_256,  packforms::cout,    25, 64},
    /* PF_W2F     */ {PACK_WINO_F,   PACK_SIDE_FWD, packforms::has_wino,    36, packforms::xi_f5,          false, false, packforms::ld_cout,    packforms::cout_256, packforms::cin,     25, 36},
    /* PF_W2D     */ {PACK_WINO_D,   PACK_SIDE_BWD, packforms::has_wino,    36, packforms::xi_d5,          false, true,  packforms::ld_cin,     packforms::cin_256,  packforms::cout,    25, 36},
};
// (rd / wr of the two stride-2 set pairs: the 16-point sets are written over the four phases, 4 x 16 = 64 floats per filter, the 36-point ones 4 x 36)

// the order the forms lie in a packed buffer (kept from before the catalogue: packed buffers stay byte-compatible)
static const PackForm kPackLayout[kNumForms] = {PF_FWD, PF_BIAS, PF_DGRAD, PF_DCLS, PF_IFWD, PF_W2F, PF_W2D, PF_W4F, PF_W4D, PF_W3D, PF_W3F, PF_W43D,
                                                PF_W43F, PF_TRUNK_T};

static inline long long form_floats(const ConvSpec& c, PackForm f) { return kPackForms[f].pts * kPackForms[f].xi(c); }
static inline long long form_xi(const ConvSpec& c, PackForm f) { return kPackForms[f].xi(c); }
static inline unsigned spec_forms(const ConvSpec& c)                       // the forms this layer has
{
    unsigned m = 0;
    for (int f = 0; f < kNumForms; ++f) if (c.off[f] >= 0) m |= 1u << f;
    return m;
}
static inline unsigned side_forms(int sides)                               // the forms a forward (1) / backward (2) pass reads
{
    unsigned m = 0;
    for (int f = 0; f < kNumForms; ++f) if (kPackForms[f].side & sides) m |= 1u << f;
    return m;
}
static inline PackForm wino_form(bool four, bool dgrad) { return four ? (dgrad ? PF_W4D : PF_W4F) : (dgrad ? PF_W2D : PF_W2F); }       // upSample1/2
static inline PackForm wino3_form(bool four, bool dgrad) { return four ? (dgrad ? PF_W43D : PF_W43F) : (dgrad ? PF_W3D : PF_W3F); }   // downSample1/2

// what a schedule needs of a layer (masks over PackForm; add_spec_jobs drops the forms the layer does not have)
// trunk fused: the layer runs on the fused trunk kernels (OIHW forward); only the transposed data-gradient copy is needed
static inline unsigned trunk_fused_forms(const ConvSpec& c) { return c.off[PF_TRUNK_T] >= 0 ? form_bit(PF_TRUNK_T) : kAllForms; }
// Winograd only: the layer runs on the Winograd kernels in every pass (forward, data-gradient); its direct K-major copies are skipped
static inline unsigned wino_only_forms(const ConvSpec& c) { return (c.wino || c.wino3) ? kAllForms & ~(form_bit(PF_FWD) | form_bit(PF_DGRAD)) : kAllForms; }
// implicit GEMM only: the layer runs on the implicit-GEMM kernels in every pass (the discriminators' stride-2 layers): the bias and the
// tap-major forward copy, which serves the forward pass and, read row-major, the data gradient
static inline unsigned igemm_only_forms(const ConvSpec& c) { return c.igemm ? form_bit(PF_BIAS) | form_bit(PF_IFWD) : kAllForms; }

// Gradient store mode (MCVC_BWD_STORE_GRADS, include/mcvc.h): the layers whose weight-gradient writers can STORE a pass's gradient instead of
// adding to what the buffer held -- the Winograd layers, the implicit-GEMM layers and the wide 1 x KW convolutions of the 1-D trunk
// (wgrad_smallk* / wgemm).  A static predicate of the layer alone: the fused update (which gradients a zero_grads == 2 update leaves
// uncleared) and conv_wgrad (which passes store) both read it, so the two can never disagree.  Biases, norm affine parameters and the edge
// layers (2 input channels / 1 output channel: the atomic writers) are not covered: they are cleared and accumulated into as before.
static inline bool grad_store_covered(const ConvSpec& c)
{
    return c.wino || c.wino3 || c.igemm || (c.KH == 1 && c.stride == 1 && c.Cin >= 64 && c.cout_tot >= 64);
}

static void spec_finalize(ConvSpec& c, long long& cur)
{
    c.cout_tot = c.Cout * c.nbr;
    c.cout_pk = round_up_i(c.cout_tot, 32);
    c.cin_pad = round_up_i(c.Cin, 2);
    c.w_rows = c.cin_pad * c.KH * c.KW;
    c.cin_pk = round_up_i(c.Cin, 32);
    c.dg_rows_co = round_up_i(c.cout_tot, 2);
    c.ncls = 0;
    const int st = c.stride;
    long long o = 0;
    for (int qh = 0; qh < st; ++qh) {
        for (int qw = 0; qw < st; ++qw) {
            DgradClass k{};
            const int khmin = (qh + c.ph) % st, kwmin = (qw + c.pw) % st;
            if (khmin > c.KH - 1 || kwmin > c.KW - 1) continue;
            k.khmax = khmin + st * ((c.KH - 1 - khmin) / st);
            k.kwmax = kwmin + st * ((c.KW - 1 - kwmin) / st);
            k.nth = (k.khmax - khmin) / st + 1;
            k.ntw = (k.kwmax - kwmin) / st + 1;
            k.pad_h = (k.khmax - qh - c.ph) / st;
            k.pad_w = (k.kwmax - qw - c.pw) / st;
            k.qh = qh; k.qw = qw;
            k.offset = o;                      // inside PF_DGRAD (stride 1) / PF_DCLS (ucls, stride 2)
            o += packforms::dgrad_class_floats(c, k);
            c.ucls[c.ncls] = c.icls[c.ncls] = k;
            c.cls[c.ncls++] = k;
        }
    }
    c.merged = 0;
    if (st == 2) {
        c.merged = 1;
        c.mg_pad_h = c.mg_pad_w = 0;
        for (int k = 0; k < c.ncls; ++k) {
            if (c.cls[k].pad_h > c.mg_pad_h) c.mg_pad_h = c.cls[k].pad_h;
            if (c.cls[k].pad_w > c.mg_pad_w) c.mg_pad_w = c.cls[k].pad_w;
        }
        c.mg_kh = c.mg_kw = 1;
        for (int k = 0; k < c.ncls; ++k) {
            DgradClass& d = c.cls[k];
            d.su = c.mg_pad_h - d.pad_h; d.sv = c.mg_pad_w - d.pad_w; d.offset = 0;
            if (d.su + d.nth > c.mg_kh) c.mg_kh = d.su + d.nth;
            if (d.sv + d.ntw > c.mg_kw) c.mg_kw = d.sv + d.ntw;
            const long long uo = c.ucls[k].offset;          // the per-class copies keep their own offsets
            c.ucls[k] = c.icls[k] = d; c.ucls[k].offset = uo;
        }
        c.mg_ld = round_up_i(4 * c.Cin, 32);
    }
    c.igemm = (st == 2 && c.KH == 3 && c.KW == 3 && c.ph == 1 && c.pw == 1 && (c.Cin % 64) == 0 && (c.cout_tot % 64) == 0 && c.ncls == 4) ? 1 : 0;
    c.wino = (c.KH == 5 && c.KW == 5 && st == 1 && c.nbr == 1 && c.Cin >= 64 && c.Cout >= 64) ? 1 : 0;
    c.wino3 = (c.merged && c.KH == 5 && c.KW == 5 && c.ph == 2 && c.pw == 2 && (4 * c.Cin) % 128 == 0 && c.cout_tot % 16 == 0) ? 1 : 0;
    for (PackForm f : kPackLayout) {
        const PackFormRow& r = kPackForms[f];
        c.off[f] = -1;
        if (r.has(c)) {
            if (r.align_before) cur = (cur + 3) & ~3LL;
            c.off[f] = cur; cur += form_floats(c, f);
        }
        if (r.align_after) cur = (cur + 3) & ~3LL;
    }
}

// ---- job tables of the whole-network re-pack and of the fused update --------------------------------------------------------------------
struct PackTable { std::vector<PackJob> jobs; std::vector<PackDgradArgs> dga; int nblocks = 0; double bytes = 0.0, wbytes = 0.0;     // wbytes: the written share
                   unsigned sides = kAllForms; };      // the forms of the side(s) this table refreshes (side_forms of `sets`)

static PackDgradArgs dgrad_args(const ConvSpec& c, int br)
{
    PackDgradArgs a{};
    a.Cin = c.Cin; a.KH = c.KH; a.KW = c.KW; a.step = c.stride; a.ld = c.merged ? c.mg_ld : c.cin_pk; a.co_off = br * c.Cout; a.ncls = c.ncls;
    a.merged = c.merged; a.mg_kh = c.mg_kh; a.mg_kw = c.mg_kw;
    for (int k = 0; k < c.ncls; ++k) a.cls[k] = c.cls[k];
    return a;
}

// the jobs that refresh `forms` of one layer (those it has, on the side(s) the table refreshes), one per branch and form
static void add_spec_jobs(PackTable& t, const ConvSpec& c, unsigned forms)
{
    const int taps = c.KH * c.KW, K = c.Cin * taps;
    forms &= spec_forms(c);
    const unsigned direct = form_bit(PF_FWD) | form_bit(PF_BIAS) | form_bit(PF_DGRAD) | form_bit(PF_TRUNK_T);
    for (int br = 0; br < c.nbr; ++br) {
        for (int f = 0; f < kNumForms; ++f) {
            if (!(forms >> f & 1)) continue;
            const PackFormRow& r = kPackForms[f];
            const bool written = (t.sides >> f & 1) != 0;
            // (kept from the hand-written accounting: a layer whose bias is scheduled counts its direct copies on BOTH sides, written or not)
            if (!written && !((direct >> f & 1) && (forms & form_bit(PF_BIAS)))) continue;
            const double n = r.kind == PACK_COPY ? (double)c.Cout : (double)c.Cout * c.Cin;
            t.bytes += 4.0 * n * ((r.rd ? r.rd : taps) + (r.wr ? r.wr : taps));
            t.wbytes += 4.0 * n * (r.wr ? r.wr : taps);
            if (!written) continue;
            PackJob j{};
            j.kind = r.kind; j.param = r.kind == PACK_COPY ? c.bi[br] : c.wi[br]; j.dst = c.off[f]; j.Cout = c.Cout; j.ld = r.ld(c);
            if (r.kind == PACK_COPY) j.dst += br * c.Cout;
            else { j.Cin = c.Cin; j.taps = taps; }              // every weight job carries its tensor's geometry: the fused update's tiles (plan_upd)
            if (r.kind != PACK_COPY && r.kind != PACK_DGRAD) j.co_off = br * c.Cout;
            if (r.pts > 1) j.xi_stride = r.xi(c);
            if (r.kind == PACK_FWD || r.kind == PACK_FWD_TAP) j.K = K;
            if (r.kind == PACK_FWD_TAP) j.KW = taps;
            if (r.kind == PACK_TRUNK_T) j.KW = c.KW;
            if (r.kind == PACK_DGRAD) {
                PackDgradArgs a = dgrad_args(c, br);
                if (f == PF_DCLS) { a.merged = 0; a.ld = c.cin_pk; for (int k = 0; k < c.ncls; ++k) a.cls[k] = c.ucls[k]; }
                j.dg = (int)t.dga.size();
                t.dga.push_back(a);
            }
            j.block0 = t.nblocks; j.gx = r.gx(c);
            t.nblocks += j.gx * r.gy(c);
            t.jobs.push_back(j);
        }
    }
}
