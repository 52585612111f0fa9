// kurbm_plan.h -- host-side planning of the C-ABI layer: the knobs, tile choice, split-K slicing, the plane formats of the x3 step
// and the layout of every caller-sized buffer.  Plain C++17, no HIP include and no device call: tests/dump_host_plans.cpp runs all
// of it on the CPU, and the kurbm_*_bytes functions of include/kurbm.h are these carvers on a null base.
#ifndef KURBM_PLAN_H
#define KURBM_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/kurbm.h"

namespace kurbm {

// operand layouts: VH  A=[m][k] B=[k][n];  HV  A=[m][k] B=[n][k];  OUTER  A=[k][m] B=[k][n]
enum { LAYOUT_VH = 0, LAYOUT_HV = 1, LAYOUT_OUTER = 2 };
// tile configurations (BM x BN, waves as WAVES_M x WAVES_N); see tile_shape()
enum { CFG_128x128 = 0, CFG_128x112 = 1, CFG_112x128 = 2, CFG_128x64 = 3, CFG_64x128 = 4, CFG_64x64 = 5,
       CFG_64x112 = 6, CFG_112x64 = 7, CFG_COUNT = 8 };
inline void tile_shape(int cfg, int* bm, int* bn) {
    static const int shapes[CFG_COUNT][2] = {{128, 128}, {128, 112}, {112, 128}, {128, 64}, {64, 128}, {64, 64}, {64, 112}, {112, 64}};
    *bm = shapes[cfg][0];
    *bn = shapes[cfg][1];
}

// Experiment knobs.  Every one is read from the environment ONCE, at kurbm_ctx_create, into the context (no getenv on
// the launch path); kurbm_ctx_set_option changes one on a live context (tests and tuning sweeps).  KN_AUTO = "let the
// planner decide".
enum { KN_LDPAD, KN_X3_F8POS, KN_X3_BYTES, KN_X3_STATS_TALL, KN_BF16_SPLIT, KN_X3_FULL, KN_X3_TALL, KN_X3_MFAST, KN_X3_STATS_MFAST,
       KN_UNFUSED_MIRROR, KN_X3_XCD2D, KN_REDUCE_TR, KN_DP_CHUNKS, KN_X3_STATS_BYTES, KN_MAP_SLOW, KN_X3_PAIR, KN_X3_SPLIT_STATS, KN_X3_ATR, KN_SMALL_LOCAL,
       KN_DISC_STAGE, KN_X3_PACKED_EPI, KN_X3_KTAIL, KN_CFG_VH, KN_CFG_HV, KN_CFG_OUTER, KN_SPLIT, KN_TILE_MAJOR, KN_COUNT };
constexpr int KN_AUTO = -1;
struct KnobRow { const char* env; int dflt; };
inline constexpr KnobRow KNOBS[KN_COUNT] = {
    {"KURBM_LDPAD", 0},            // extra elements per bf16 plane row (L2 channel camping probe: no effect)
    {"KURBM_X3_F8POS", 1},         // 0: the positive statistics of 0/1 data stay on bf16 planes
    {"KURBM_X3_BYTES", 1},         // 0: the row-major planes of 0/1 samples / data stay bf16 (1: bytes, half the A tiles)
    {"KURBM_X3_STATS_TALL", 1},    // 0: 128 x 128 tiles for the x3 statistics GEMM (1: 256 x 64 where n_vis > 128)
    {"KURBM_BF16_SPLIT", KN_AUTO}, // split-K slices of the bf16 / x3 statistics GEMM
    {"KURBM_X3_FULL", 0},          // 1: all nine piece pairs of a real x real product
    {"KURBM_X3_TALL", KN_AUTO},    // 0 / 1: never / always 256 x 64 half-step tiles
    {"KURBM_X3_MFAST", 1},         // block order of the x3 half steps
    {"KURBM_X3_STATS_MFAST", 0},   // block order of the x3 statistics GEMM
    {"KURBM_UNFUSED_MIRROR", 0},   // 1: slab reduce and weight-piece mirror as two launches
    {"KURBM_X3_XCD2D", 1},         // 0: linear block order of k_gemm_pb instead of one 2-D block of tiles per XCD
    {"KURBM_REDUCE_TR", 0},        // tile height (16 / 32 / 64) of the slab-reduce + mirror launch; 0: by the grid it makes
    {"KURBM_DP_CHUNKS", 0},        // row ranges of dW in the data-parallel step when the caller passes n_chunks <= 0; 0: by message size
    {"KURBM_X3_STATS_BYTES", 1},   // 0: v_neg^T reaches the statistics GEMM as a bf16 plane (1: as bytes where the positive half is fp8)
    {"KURBM_MAP_SLOW", 0},         // 1: k_gemm_pb maps its blocks by integer division (the path of grids too large for the multiply-high
                                   //    constants: tests)
    {"KURBM_X3_PAIR", 1},          // 0: a real-valued A operand walks its three segments one after the other (256 x 64 tiles, the generic walk);
                                   //    1: two tiles per k position on 128 x 128 tiles (k_gemm_pb, "BSP")
    {"KURBM_X3_SPLIT_STATS", 1},   // 0: the statistics of real-valued data in ONE launch (round 3: three one-piece positive tiles per k position);
                                   //    1: two launches -- the positive half as the transposed problem h_pos^T (bytes) x the pieces of v_pos^T, the
                                   //    negative half on byte planes (Bernoulli visibles) or on the paired walk (Gaussian visibles)
    {"KURBM_X3_ATR", 1},           // 0: Gaussian visibles leave the h -> v half step as pieces in BOTH orientations; 1: row-major only, and the
                                   //    negative statistics read them through transposed LDS reads (with KURBM_X3_SPLIT_STATS)
    {"KURBM_SMALL_LOCAL", 1},      // 1: the one-launch small step hands h_pos / v_neg between the workgroups of ONE XCD through its L2 (kurbm_small.hip;
                                   //    where the context's probe found the dispatcher dealing consecutive workgroups to consecutive XCDs), 0: every phase over the whole grid
    {"KURBM_DISC_STAGE", 0},       // measurement (tools/disc_times.py): the launches kurbm_class_grad makes, on the planes a complete call left in its
                                   //    workspace -- 0: all; 1: the linear half step and k_class_logits; 2: k_class_grad alone; 3: the statistics GEMM,
                                   //    its slab reduction and k_class_reduce.  kurbm_disc_step / kurbm_disc_epoch do not read it
    {"KURBM_X3_PACKED_EPI", 1},    // 0: a Bernoulli half step that leaves byte planes builds them from fp32 1.0 / 0.0 per element (the general
                                   //    epilogue of k_gemm_pb); 1: from packed bytes, four rows of a column per dword (the same planes, bit for bit)
    {"KURBM_X3_KTAIL", 1},         // 0: a half step on a byte A plane multiplies the whole last k-tile; 1: where the units end in the tile's first
                                   //    k-step (round_up(n, 32) < round_up(n, 64): 784 visibles) the second one, all padding, is skipped (exact)
    {"KURBM_CFG_VH", KN_AUTO},     // fp32 path: the tile configuration (CFG_*) of the v -> h half steps,
    {"KURBM_CFG_HV", KN_AUTO},     // ... of the h -> v half steps,
    {"KURBM_CFG_OUTER", KN_AUTO},  // ... of the statistics GEMM (these three in the order of LAYOUT_*)
    {"KURBM_SPLIT", KN_AUTO},      // fp32 path: split-K slices of the statistics GEMM
    {"KURBM_TILE_MAJOR", 1},       // fp32 path: the k-slices of a statistics tile share an XCD
};

// What planning reads of a context.  kurbm_ctx embeds it; a test fills one by hand.
struct PlanCtx {
    int ncu;
    int knob[KN_COUNT];
};
inline void plan_ctx_init(PlanCtx* c, int ncu) {
    c->ncu = ncu;
    for (int i = 0; i < KN_COUNT; ++i) c->knob[i] = KNOBS[i].dflt;
}
inline bool plan_ctx_set(PlanCtx* c, const char* name, int value) {
    for (int i = 0; i < KN_COUNT; ++i)
        if (strcmp(name, KNOBS[i].env) == 0) { c->knob[i] = value; return true; }
    return false;
}
inline int force_cfg(const PlanCtx* c, int layout) { return c->knob[KN_CFG_VH + layout]; }

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline size_t align_up(size_t x) { return (x + 255) / 256 * 256; }
// Leading dimension of a bf16 plane = its k extent (+ KURBM_LDPAD elements: an experiment knob.  Row strides
// that are multiples of 2 KiB were suspected of camping on one L2 channel; padding them changed nothing.)
inline int ld_pad(const PlanCtx* ctx, int k) { return k + ctx->knob[KN_LDPAD]; }

// ---- tiles and split-K -------------------------------------------------------------------
// Tile choice for an M x N output.  Model, fitted to MI355X measurements of this kernel family
// (profiles/): time ~ padded MFMA work x CU imbalance / efficiency, where a CU that holds
// two or more workgroups (their barriers and epilogues interleave) runs ~0.70 MFMA-busy and a CU
// with a single workgroup ~0.62.  Ties go to the larger tile (less L2 -> LDS traffic).
inline int pick_cfg(int ncu, int M, int N, int* gm_out, int* gn_out, int force = -1) {
    int best = 0;
    double best_cost = -1.0;
    long long best_blocks = 0;
    for (int c = 0; c < CFG_COUNT; ++c) {
        if (force >= 0 && force < CFG_COUNT && c != force) continue;
        int bm, bn;
        tile_shape(c, &bm, &bn);
        const long long blocks = (long long)ceil_div(M, bm) * ceil_div(N, bn);
        const long long per_cu = (blocks + ncu - 1) / ncu;                 // what the busiest CU runs
        const double eff = (blocks >= 2LL * ncu) ? 0.70 : (blocks > ncu ? 0.66 : 0.62);
        const double cost = (double)per_cu * bm * bn / eff;
        if (best_cost < 0 || cost < best_cost * 0.999 || (cost <= best_cost * 1.001 && blocks < best_blocks)) {
            best = c; best_cost = cost; best_blocks = blocks;
        }
    }
    int bm, bn;
    tile_shape(best, &bm, &bn);
    *gm_out = ceil_div(M, bm);
    *gn_out = ceil_div(N, bn);
    return best;
}

// A statistics GEMM: tile configuration and grid, k-tiles per segment and in all, and their split-K slicing
struct OuterPlan { int cfg, gm, gn, nkt, kt_total, nsplit, nsplit_bound, kt_per_split, ld_slab; };

// The slicing of every statistics plan: kt_total k-tiles as at most min(s, s_cap) slices, each a multiple of `granule` tiles.
// nsplit_bound is what a workspace reserves (it does not shrink when the rounding leaves fewer slices), nsplit what a launch runs.
inline void slice_k(OuterPlan& pl, int kt_total, int s, int s_cap, int granule) {
    if (s > s_cap) s = s_cap;
    if (s < 1) s = 1;
    pl.kt_total = kt_total;
    pl.nsplit_bound = s;
    pl.kt_per_split = kt_total > 0 ? round_up(ceil_div(kt_total, s), granule) : 0;
    pl.nsplit = kt_total > 0 ? ceil_div(kt_total, pl.kt_per_split) : 1;
}

// fp32 statistics GEMM: output n_vis x n_hid, k = batch rows in nseg signed segments (2: v_pos^T.h_pos - v_neg^T.h_neg; 1: the pixel
// rows of the discriminative gradient, v_pix^T.g -- k_gemm's walk takes nseg = 1 as it stands: its segment index is t >= nkt, which
// no tile reaches)
inline OuterPlan plan_outer(const PlanCtx* ctx, int rows, int n_vis, int n_hid, int nseg = 2) {
    OuterPlan pl;
    // tile by least padded area (independent of rows so the slab count is monotone in rows)
    long long best = -1;
    pl.cfg = 0; pl.gm = pl.gn = 1;
    const int fc = force_cfg(ctx, LAYOUT_OUTER);
    for (int c = (fc >= 0 ? fc : 0); c < (fc >= 0 ? fc + 1 : 3); ++c) {
        int bm, bn;
        tile_shape(c, &bm, &bn);
        const int gm = ceil_div(n_vis, bm), gn = ceil_div(n_hid, bn);
        const long long area = (long long)gm * gn * bm * bn;
        if (best < 0 || area < best) { best = area; pl.cfg = c; pl.gm = gm; pl.gn = gn; }
    }
    pl.nkt = rows / 32;          // full k-tiles per segment; a rows % 32 tail goes to the last slice
    // two workgroups per CU: their barriers / slab stores interleave (measured 8-10 % over one per CU)
    const int s = ctx->knob[KN_SPLIT] > 0 ? ctx->knob[KN_SPLIT] : (2 * ctx->ncu) / (pl.gm * pl.gn);
    slice_k(pl, nseg * pl.nkt, s, nseg * pl.nkt, 1);
    pl.ld_slab = round_up(n_hid, 4);
    return pl;
}
inline OuterPlan plan_outer_one(const PlanCtx* ctx, int rows, int m, int n_hid) { return plan_outer(ctx, rows, m, n_hid, 1); }

// the bf16 / x3 statistics GEMM on k_gemm_pb: k-tile 64, one workgroup per CU, `per` tiles per k position walked fastest, so a slice
// is a whole number of `granule` tiles; at most s_max slices (a row range keeps inside the slab memory carved for the whole matrix)
inline void slice_k_pb(const PlanCtx* ctx, OuterPlan& pl, int n_hid, int per, int s_max, int s_cap, int granule) {
    const int s = ctx->knob[KN_BF16_SPLIT] != KN_AUTO ? ctx->knob[KN_BF16_SPLIT] : ctx->ncu / (pl.gm * pl.gn);
    slice_k(pl, per * pl.nkt, s, s_max < s_cap ? s_max : s_cap, granule);
    pl.ld_slab = round_up(n_hid, 4);
}
inline OuterPlan plan_outer_bf16(const PlanCtx* ctx, int rows, int n_vis, int n_hid, int nseg, int s_max = 1 << 30,
                                 bool f8pos = false, bool x3 = false, int n_vis_whole = 0) {
    OuterPlan pl;
    // n_vis_whole: this plan is for a ROW RANGE of a matrix of that many visible rows -- it keeps the whole matrix's tile shape, which
    // the planes were written for (the byte-plane statistics of 0/1 data exist on the 256 x 64 tile only: a range of <= 128 rows
    // planned for itself came out as 128 x 128 and the launch was refused, hipErrorInvalidValue)
    if (n_vis_whole < n_vis) n_vis_whole = n_vis;
    // x3: 256 x 64 tiles -- the three-piece B tile is the heavy operand (3 x 8 KB against 3 x 16), so a k-tile is 56 KB instead
    // of 64 for the same MFMAs, and 784 x 1024 fills 256 workgroups instead of 224 (statistics GEMM 28.5 -> 27.4 us)
    pl.cfg = (x3 && ctx->knob[KN_X3_STATS_TALL] != 0 && n_vis_whole > 128) ? 2 : 0;
    pl.gm = ceil_div(n_vis, pl.cfg == 2 ? 256 : 128);
    pl.gn = ceil_div(n_hid, pl.cfg == 2 ? 64 : 128);
    // f8pos: the walk is in units of 128 k -- one fp8 tile of segment 0, two 64-deep tiles of every other segment
    const int per = f8pos ? 2 * nseg - 1 : nseg;
    pl.nkt = round_up(rows, 128) / (f8pos ? 128 : 64);
    slice_k_pb(ctx, pl, n_hid, per, s_max, pl.nkt, per);
    return pl;
}

// The statistics of REAL-VALUED data (x3, v_pieces = 3) as two launches (KURBM_X3_SPLIT_STATS).
//   positive:  the transposed problem -- A = h_pos^T [n_hid][batch] as a k-permuted byte plane, B = the three pieces of v_pos^T
//              [n_vis][batch]; 256 x 64 tiles of (hidden x visible) that leave transposed into ordinary slabs;
//   negative:  Bernoulli visibles: A = v_neg^T as bytes, B = the pieces of -h_neg^T, 256 x 64 tiles (the plain byte-plane walk);
//              Gaussian visibles: A = the three pieces of v_neg^T, B = those of -h_neg^T, 128 x 128 tiles on the paired walk.
// Each launch cuts k into slices of whole 128-deep blocks (two k positions) so that its grid fills the chip; the slabs of both are
// summed by the one reduce launch (negative slabs first).
struct SplitStats { OuterPlan pos, neg; };
inline SplitStats plan_split_stats(const PlanCtx* ctx, int rows, int n_vis, int n_hid, bool gauss, int s_max = 1 << 30) {
    SplitStats sp;
    auto fill = [&](OuterPlan& pl, int gm, int gn, int cfg, int per) {
        pl.gm = gm; pl.gn = gn; pl.cfg = cfg;
        pl.nkt = round_up(rows, 128) / 64;
        slice_k_pb(ctx, pl, n_hid, per, s_max, pl.nkt / 2, 2 * per);
    };
    fill(sp.pos, ceil_div(n_hid, 256), ceil_div(n_vis, 64), 2, 1);
    if (gauss) fill(sp.neg, ceil_div(n_vis, 128), ceil_div(n_hid, 128), 0, 3);
    else fill(sp.neg, ceil_div(n_vis, 256), ceil_div(n_hid, 64), 2, 1);
    return sp;
}

// ---- the plane formats of a bf16 / x3 step ------------------------------------------------
// Computed once from (knobs, pieces, the caller's v_pieces with its KURBM_V_BINARY bit, mode, n_vis); the step, the score, the
// conversion of resident planes, the Gibbs workspace and the plane dump of the tests all read THIS value.
struct PlaneFormats {
    bool v_binary, gauss;
    int v_pieces;        // without the KURBM_V_BINARY bit
    int vn_pieces;       // x3 with Gaussian visibles: v_t / v_neg are real-valued, so they travel as three pieces like real-valued data
    bool f8pos;          // 0/1 data on the x3 path: v_pos^T and h_pos^T leave as fp8 planes and their product runs on the fp8 matrix cores
    // ... and every row-major plane of 0/1 values is a BYTE plane (half the A tile of the half step that reads it): the hidden
    // samples always, v_pos / the persistent chain for 0/1 data, the negative visibles in Bernoulli mode (the rounded-bf16 path
    // too: its 0/1 states are exact as bytes, so nothing changes but the bytes the half steps stage)
    bool hbytes, vbytes, nbytes;
    // ... and v_neg^T, the A operand of the statistics GEMM's negative half, where the positive half runs on fp8 planes (the
    // walk is then whole units of fp8 / 3-piece / 3-piece tiles: k_gemm_pb<..., EPI_SLAB, ..., AB>): 32 KB per 128 k, not 64
    bool tbytes;
    bool split_stats;    // real-valued data: the statistics as two launches (plan_split_stats), h_pos^T -- and v_neg^T of Bernoulli visibles -- as byte planes
    bool tbytes_n;       // v_neg^T is a byte plane (either reason)
    // ... and Gaussian visibles need no transposed copy of v_neg at all: the paired walk of the negative statistics reads the row-major
    // pieces through transposed LDS reads (k_gemm_pb, "ATR"); needs the paired walk on 128 x 128 tiles, whose LDS rows are then the
    // plane's 128-column blocks (n_vis padded to 128 = the plane's ld)
    bool vneg_tr;
};
inline PlaneFormats plane_formats(const PlanCtx* ctx, int pieces, int v_pieces, int mode, int n_vis) {
    const int* kn = ctx->knob;
    PlaneFormats f;
    f.v_binary = v_pieces == (1 | KURBM_V_BINARY);
    f.v_pieces = f.v_binary ? 1 : v_pieces;
    f.gauss = mode == KURBM_MODE_VISIBLE_GAUSSIAN;
    f.vn_pieces = (pieces == 3 && f.gauss) ? 3 : 1;
    const bool byt = kn[KN_X3_BYTES] != 0;
    f.f8pos = f.v_binary && pieces == 3 && kn[KN_X3_F8POS] != 0;
    f.hbytes = byt; f.vbytes = byt && f.v_binary && pieces == 3; f.nbytes = byt && !f.gauss;
    f.tbytes = f.f8pos && f.nbytes && kn[KN_X3_STATS_BYTES] != 0 && kn[KN_X3_STATS_TALL] != 0 && n_vis > 128;
    f.split_stats = pieces == 3 && f.v_pieces == 3 && kn[KN_X3_SPLIT_STATS] != 0 && byt;
    f.tbytes_n = f.tbytes || (f.split_stats && f.nbytes);
    f.vneg_tr = f.gauss && f.split_stats && kn[KN_X3_ATR] != 0 && kn[KN_X3_PAIR] != 0 && kn[KN_LDPAD] == 0;
    return f;
}

// ---- carving -----------------------------------------------------------------------------
// A caller-sized buffer handed out front to back in 256-byte-aligned members.  It tracks the OFFSET: on a null base every member
// is null and `off` is still the size (the kurbm_*_bytes queries), and no arithmetic is ever done on a null pointer.
struct Arena {
    uintptr_t base;
    size_t off = 0;
    explicit Arena(const void* b) : base(reinterpret_cast<uintptr_t>(b)) {}
    template <class T> T* take(size_t n) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off = align_up(off + n * sizeof(T));
        return p;
    }
};

constexpr int SMALL_ROWS_MAX = 512;   // batches up to here carry the transposed planes of the one-launch step in their workspace

struct Workspace {
    float *h_pos, *h_neg, *h_tmp, *v_neg, *part_h, *part_v, *slab;
    float *small_t;   // kurbm_cd_step_small's transposed planes (rows <= SMALL_ROWS_MAX only)
    int ldh, ldv, ld_part_h, ld_part_v, max_row_tiles;
    size_t slab_stride, bytes;
};
// ldv_batch (kurbm_cd_step only): the leading dimension of the caller's batch.  The step keeps v_neg at THAT leading dimension (the
// statistics GEMM takes v_pos and v_neg as the two segments of one operand, with one lda), so a batch wider than round_up(n_vis, 4)
// needs rows * (ldv - round_up(n_vis, 4)) more floats here than kurbm_workspace_bytes reports: include/kurbm.h has the formula.
inline Workspace carve_f32(const PlanCtx* ctx, void* base, int rows, int n_vis, int n_hid, int ldv_batch = 0) {
    Workspace w;
    w.ldh = round_up(n_hid, 4);
    w.ldv = round_up(n_vis, 4);
    w.max_row_tiles = ceil_div(rows, 64);
    w.ld_part_h = w.ldh;
    w.ld_part_v = w.ldv;
    const OuterPlan pl = plan_outer(ctx, rows, n_vis, n_hid);
    w.slab_stride = (size_t)n_vis * pl.ld_slab;
    Arena ar(base);
    w.h_pos = ar.take<float>((size_t)rows * w.ldh);
    w.h_neg = ar.take<float>((size_t)rows * w.ldh);
    w.h_tmp = ar.take<float>((size_t)rows * w.ldh);   // intermediate h_t (k > 1) / persistent-chain start
    w.v_neg = ar.take<float>((size_t)rows * (ldv_batch > w.ldv ? ldv_batch : w.ldv));
    w.part_h = ar.take<float>((size_t)w.max_row_tiles * w.ld_part_h);
    w.part_v = ar.take<float>((size_t)w.max_row_tiles * w.ld_part_v);
    w.slab = ar.take<float>(w.slab_stride * pl.nsplit_bound);
    // (the one-launch score keeps its row partials there: 2 ceil(n_hid / 16) + ceil(n_vis / 16) + 1 rows -- the + 4 covers one-unit layers)
    w.small_t = rows <= SMALL_ROWS_MAX ? ar.take<float>((size_t)(2 * n_hid + n_vis + 4) * round_up(rows, 16)) : nullptr;
    // free energy: row partials [col tiles][round_up(rows,4)] alias the front of the workspace
    const size_t fe = align_up((size_t)ceil_div(n_hid, 64) * round_up(rows, 4) * 4);
    w.bytes = ar.off > fe ? ar.off : fe;
    return w;
}

// Annealed importance sampling, a run on `rows` chains: the chain state v, the hidden plane h, and the row partials of both GEMM
// launches (one row of partials per group of 16 columns).  kurbm_ais_step uses the partials only.
struct AisWorkspace {
    float *v, *h, *sppart, *vpart;
    int ldv, ldh, ld_part, ng_h, ng_v;
    size_t bytes;
};
// n_labels > 0 (kurbm_ais_run_labels): the h -> v launch covers the n_pix = n_vis - n_labels pixel columns and the label site adds ONE
// group row behind their ceil(n_pix / 16) -- which can be one more than ceil(n_vis / 16) (n_pix = 33, C = 2).
inline AisWorkspace carve_ais(void* base, int rows, int n_vis, int n_hid, int n_labels = 0) {
    AisWorkspace w;
    w.ldv = round_up(n_vis, 4);
    w.ldh = round_up(n_hid, 4);
    w.ld_part = round_up(rows, 4);
    w.ng_h = ceil_div(n_hid, 16);
    w.ng_v = n_labels > 0 ? ceil_div(n_vis - n_labels, 16) + 1 : ceil_div(n_vis, 16);
    Arena ar(base);
    w.v = ar.take<float>((size_t)rows * w.ldv);
    w.h = ar.take<float>((size_t)rows * w.ldh);
    w.sppart = ar.take<float>((size_t)w.ng_h * w.ld_part);
    w.vpart = ar.take<float>((size_t)w.ng_v * w.ld_part);
    w.bytes = ar.off;
    return w;
}

// kurbm_class_logits: the pre-activation plane a [rows][round_up(n_hid, 4)]
struct ClassWorkspace { float* a; int lda; size_t bytes; };
inline ClassWorkspace carve_class(void* base, int rows, int n_hid) {
    ClassWorkspace w;
    w.lda = round_up(n_hid, 4);
    Arena ar(base);
    w.a = ar.take<float>((size_t)rows * w.lda);
    w.bytes = ar.off;
    return w;
}

// Discriminative / hybrid step on `rows` rows: the pre-activation plane, logits and posterior, the gradient plane g, nll, the row-tile
// partials (tiles of DISC_TILE_ROWS rows: kurbm_classgrad.hip), the slabs of the pixel-row statistics GEMM, two packed deltas (the
// step's own and the generative one) and, LAST, the workspace of the generative chain (carve_f32; a batch wider than
// round_up(n_vis, 4) grows it as it does there).
constexpr int DISC_TILE_ROWS = 32, DISC_PART_D = 64;   // = CG_ROWS, CG_PART_D of kurbm_kernels.h (asserted where both are seen)
struct DiscWorkspace {
    float *a, *logits, *prob, *g, *nll, *part, *part_d, *slab, *delta, *gen;
    void* cd;
    int ldh, ldl, ld_part, ntiles;
    size_t slab_stride, cd_bytes, bytes;
};
inline DiscWorkspace carve_disc(const PlanCtx* ctx, void* base, int rows, int n_vis, int n_hid, int C, int ldv_batch = 0) {
    DiscWorkspace w;
    const int n_pix = n_vis - C;
    w.ldh = round_up(n_hid, 4);
    w.ldl = round_up(C, 4);
    w.ld_part = w.ldh;
    w.ntiles = ceil_div(rows, DISC_TILE_ROWS);
    const OuterPlan pl = plan_outer_one(ctx, rows, n_pix, n_hid);
    w.slab_stride = (size_t)n_pix * pl.ld_slab;
    const size_t packed = (size_t)n_vis * n_hid + n_hid + n_vis;
    Arena ar(base);
    w.a = ar.take<float>((size_t)rows * w.ldh);
    w.logits = ar.take<float>((size_t)rows * w.ldl);
    w.prob = ar.take<float>((size_t)rows * w.ldl);
    w.g = ar.take<float>((size_t)rows * w.ldh);
    w.nll = ar.take<float>((size_t)rows);
    w.part = ar.take<float>((size_t)w.ntiles * (C + 1) * w.ld_part);
    w.part_d = ar.take<float>((size_t)w.ntiles * DISC_PART_D);
    w.slab = ar.take<float>(w.slab_stride * pl.nsplit_bound);
    w.delta = ar.take<float>(packed);
    w.gen = ar.take<float>(packed);
    w.cd_bytes = carve_f32(ctx, nullptr, rows, n_vis, n_hid, ldv_batch).bytes;
    w.cd = ar.take<char>(w.cd_bytes);
    w.bytes = ar.off;
    return w;
}

// A layer's backward pass on `rows` rows (kurbm_backprop_layer; n_in x n_out = the layer's n_vis x n_hid): the row-tile partials of
// db_h (tiles of BACKPROP_TILE_ROWS rows: kurbm_backprop.hip) FIRST -- kurbm_backprop_delta, the site alone, uses nothing else and
// takes the query at n_in = 1 -- then the slabs of the statistics GEMM x_in^T.delta.
constexpr int BACKPROP_TILE_ROWS = 16;   // = BP_ROWS of kurbm_kernels.h (asserted where both are seen)
struct BackpropWorkspace {
    float *part, *slab;
    int ld_part, ntiles;
    size_t slab_stride, bytes;
};
inline BackpropWorkspace carve_backprop(const PlanCtx* ctx, void* base, int rows, int n_in, int n_out) {
    BackpropWorkspace w;
    w.ld_part = round_up(n_out, 4);
    w.ntiles = ceil_div(rows, BACKPROP_TILE_ROWS);
    const OuterPlan pl = plan_outer_one(ctx, rows, n_in, n_out);
    w.slab_stride = (size_t)n_in * pl.ld_slab;
    Arena ar(base);
    w.part = ar.take<float>((size_t)w.ntiles * w.ld_part);
    w.slab = ar.take<float>(w.slab_stride * pl.nsplit_bound);
    w.bytes = ar.off;
    return w;
}

// The weight mirror of the bf16 / x3 paths: `pieces` bf16 planes of W and of W^T, k-padded to 128
struct Mirror { uint16_t *Wb, *Wtb; int Kh, Kv, ldW, ldWt, pieces; size_t planeW, planeWt, bytes; };
inline Mirror carve_mirror(const PlanCtx* ctx, void* base, int n_vis, int n_hid, int pieces) {
    Mirror m;
    m.pieces = pieces;
    m.Kh = round_up(n_hid, 128);   // k extent of W  [n_vis][Kh]   (B operand of h->v)
    m.Kv = round_up(n_vis, 128);   // k extent of Wt [n_hid][Kv]   (B operand of v->h)
    m.ldW = ld_pad(ctx, m.Kh);
    m.ldWt = ld_pad(ctx, m.Kv);
    m.planeW = (size_t)n_vis * m.ldW;
    m.planeWt = (size_t)n_hid * m.ldWt;
    Arena ar(base);
    m.Wb = ar.take<uint16_t>(pieces * m.planeW);
    m.Wtb = ar.take<uint16_t>(pieces * m.planeWt);
    m.bytes = ar.off;
    return m;
}

struct WorkspaceB {
    uint16_t *vb, *vbT, *hb, *hbT, *v2b, *v2bT, *h2b, *hnT, *cb;
    float *part_h, *part_v, *slab, *tmp32;
    float* rowpart;     // kurbm_score_x3's row partials
    int Kv, Kh, Kb, Lv, Lh, Lb, ldh32, ldv32, max_row_tiles;   // K*: k extents; L*: leading dimensions of the bf16 planes
    size_t planeV, planeVT, planeHT;   // distance between the pieces of v_pos (both images) and of h_neg^T
    size_t slab_stride, bytes;
};
inline WorkspaceB carve_bf16(const PlanCtx* ctx, void* base, int rows, int n_vis, int n_hid, int pieces, int v_pieces) {
    WorkspaceB w;
    w.Kv = round_up(n_vis, 128);
    w.Kh = round_up(n_hid, 128);
    w.Kb = round_up(rows, 128);
    w.Lv = ld_pad(ctx, w.Kv); w.Lh = ld_pad(ctx, w.Kh); w.Lb = ld_pad(ctx, w.Kb);
    w.ldh32 = round_up(n_hid, 4);
    w.ldv32 = round_up(n_vis, 4);
    w.max_row_tiles = ceil_div(rows, 128);
    w.planeV = (size_t)w.Kb * w.Lv;
    w.planeVT = (size_t)n_vis * w.Lb;
    w.planeHT = (size_t)n_hid * w.Lb;
    const OuterPlan pl = plan_outer_bf16(ctx, rows, n_vis, n_hid, pieces == 3 ? v_pieces + 1 : 2, 1 << 30, false, pieces == 3);
    w.slab_stride = (size_t)n_vis * pl.ld_slab;
    Arena ar(base);
    w.vb = ar.take<uint16_t>(v_pieces * w.planeV);                       // v_pos, both orientations
    w.vbT = ar.take<uint16_t>(v_pieces * w.planeVT);
    w.hb = ar.take<uint16_t>((size_t)w.Kb * w.Lh);                       // h_pos
    w.hbT = ar.take<uint16_t>((size_t)n_hid * w.Lb);
    w.v2b = ar.take<uint16_t>((pieces == 3 ? 3 : 1) * w.planeV);         // v_t / v_neg (x3: room for the three
    w.v2bT = ar.take<uint16_t>((pieces == 3 ? 3 : 1) * w.planeVT);       //  pieces of Gaussian visibles)
    w.h2b = ar.take<uint16_t>((size_t)w.Kb * w.Lh);                      // h_t (k > 1, chain start)
    w.hnT = ar.take<uint16_t>(pieces * w.planeHT);                       // h_neg probabilities, transposed
    w.cb = ar.take<uint16_t>(v_pieces * w.planeV);                       // persistent chain as bf16
    // bias partials.  bf16: one row per row tile.  x3: hidden = rows of +sum(h_pos) then rows of -sum(h_neg);
    // visible = one row per 64-row band of v_pos (conversion kernel) then rows of -sum(v_neg)
    // (k_gemm_pb writes one row per 64-row half of a 128-row tile: two rows per tile)
    w.part_h = ar.take<float>((size_t)4 * w.max_row_tiles * w.ldh32);
    w.part_v = ar.take<float>((size_t)(ceil_div(rows, 64) + 2 * w.max_row_tiles) * w.ldv32);
    int nslab_res = pl.nsplit_bound;
    if (pieces == 3 && v_pieces == 3) {   // (the mode is not known here: room for either negative launch)
        const SplitStats b = plan_split_stats(ctx, rows, n_vis, n_hid, false), gs = plan_split_stats(ctx, rows, n_vis, n_hid, true);
        const int need = b.pos.nsplit_bound + (b.neg.nsplit_bound > gs.neg.nsplit_bound ? b.neg.nsplit_bound : gs.neg.nsplit_bound);
        if (need > nslab_res) nslab_res = need;
    }
    w.slab = ar.take<float>(w.slab_stride * nslab_res);
    w.tmp32 = ar.take<float>((size_t)rows * (w.ldh32 > w.ldv32 ? w.ldh32 : w.ldv32));       // fp32 plane for the test hook
    // the score of fit(verbose = 1): softplus row partials of F(v) and F(v') per 64-column tile, |F - F'| per row
    w.rowpart = ar.take<float>((size_t)(2 * ceil_div(n_hid, 64) + 1) * round_up(rows, 4));
    w.bytes = ar.off;
    return w;
}

// The statistics GEMM(s) of a bf16 / x3 step on visible rows [m_lo, m_hi) -- all of them in a whole step, a row range in
// kurbm_x3_stats_rows.  A range keeps inside the slab memory carved for the whole matrix (each half of a two-launch form in half of it).
struct StatsPlan {
    int nseg;             // segments of the one-launch form: (piece of v_pos) x h_pos, then v_neg x (piece of -h_neg)
    OuterPlan pl;         // the one-launch form (and ld_slab of either)
    SplitStats sps;       // the two-launch form (PlaneFormats::split_stats)
    size_t slab_stride;
};
inline StatsPlan plan_stats(const PlanCtx* ctx, int pieces, int v_pieces, int mode, int rows, int n_vis, int n_hid, int m_lo, int m_hi) {
    const PlaneFormats pf = plane_formats(ctx, pieces, v_pieces, mode, n_vis);
    const size_t whole_stride = (size_t)n_vis * round_up(n_hid, 4);      // (WorkspaceB::slab_stride)
    const int Mr = m_hi - m_lo;
    StatsPlan st;
    st.nseg = pieces == 3 ? pf.v_pieces + pf.vn_pieces : 2;
    st.pl = plan_outer_bf16(ctx, rows, n_vis, n_hid, st.nseg, 1 << 30, pf.f8pos, pieces == 3);
    st.sps = plan_split_stats(ctx, rows, n_vis, n_hid, pf.gauss);
    st.slab_stride = whole_stride;
    if (Mr != n_vis) {
        st.slab_stride = (size_t)Mr * st.pl.ld_slab;
        const int s_max = (int)((whole_stride * st.pl.nsplit_bound) / st.slab_stride);
        const int s_max2 = (int)((whole_stride * (size_t)(st.sps.neg.nsplit_bound + st.sps.pos.nsplit_bound)) / st.slab_stride / 2);
        st.pl = plan_outer_bf16(ctx, rows, Mr, n_hid, st.nseg, s_max, pf.f8pos, pieces == 3, n_vis);
        st.sps = plan_split_stats(ctx, rows, Mr, n_hid, pf.gauss, s_max2);
    }
    return st;
}

// The bf16 planes of a window of `rows` data rows, as the x3 step reads them: pieces of v row-major [Kb][Lv] (A operand of
// the first half step), transposed [n_vis][Lb] (A operand of the positive statistics), and the column sums of each 64-row
// band (the positive half of db_v).  Same extents as the v_pos planes of a workspace carved for `rows` rows, so a step can
// read them IN PLACE OF its own conversion (kurbm_cd_opts::v_planes): the data matrix is static for a whole fit().
struct VPlanes { uint16_t *vb, *vbT; float* part_v; size_t bytes; };
inline VPlanes carve_vplanes(const PlanCtx* ctx, const void* base, int rows, int n_vis, int v_pieces) {
    VPlanes v;
    const int Kv = round_up(n_vis, 128), Kb = round_up(rows, 128);
    const size_t planeV = (size_t)Kb * ld_pad(ctx, Kv), planeVT = (size_t)n_vis * ld_pad(ctx, Kb);
    Arena ar(base);
    v.vb = ar.take<uint16_t>(v_pieces * planeV);
    v.vbT = ar.take<uint16_t>(v_pieces * planeVT);
    v.part_v = ar.take<float>((size_t)ceil_div(rows, 64) * round_up(n_vis, 4));
    v.bytes = ar.off;
    return v;
}

// kurbm_free_energy_x3: the bf16 pieces of v [Kb][Lp], then the row partials [column tiles of 128][round_up(rows, 4)] (the last
// member's end is not rounded up); never less than the step's workspace -- the contract is one size for every call on these rows
struct FeX3Workspace { uint16_t* Ab; float* rowpart; int Lp, Kb, grid_m, grid_n, ld_rowpart; size_t plane, bytes; };
inline FeX3Workspace carve_fe_x3(const PlanCtx* ctx, void* base, int rows, int n_vis, int n_hid, int v_pieces) {
    FeX3Workspace f;
    f.Lp = ld_pad(ctx, round_up(n_vis, 128)); f.Kb = round_up(rows, 128);
    f.plane = (size_t)f.Kb * f.Lp;
    f.grid_m = ceil_div(rows, 128); f.grid_n = ceil_div(n_hid, 128);
    f.ld_rowpart = round_up(rows, 4);
    Arena ar(base);
    f.Ab = ar.take<uint16_t>(v_pieces * f.plane);
    f.rowpart = ar.take<float>(0);
    f.bytes = ar.off + (size_t)f.grid_n * f.ld_rowpart * 4;
    const size_t query = carve_bf16(ctx, nullptr, rows, n_vis, n_hid, 3, v_pieces).bytes;
    if (query > f.bytes) f.bytes = query;
    return f;
}

// Gibbs run on `rows` chains: the converted start plane v0 (kept for the whole run: clamped units are copied back from it), the
// current visible plane vc, the hidden plane hb, and the clamp mask in the order of a plane row's positions.  Formats:
//   Gaussian visibles    v0 and vc are three bf16 pieces (a start that is exactly bf16 has zero mid / lo pieces);
//   Bernoulli, 0/1 start v0 and vc are k-permuted byte planes (one bf16 piece with KURBM_X3_BYTES = 0);
//   Bernoulli, real start (v_pieces 1 or 3): v0 is v_pieces bf16 pieces; vc is a byte plane -- unless units are clamped: the
//                        clamped values are real, so vc then keeps v0's format (its 0/1 samples have zero mid / lo pieces).
// The size does not depend on whether a mask is given: vc is carved for the larger case.
struct GibbsWorkspace {
    uint16_t *v0, *vc, *hb;
    unsigned char* maskp;
    int Kv, Kh, Kb, Lv, Lh, sp, cp;
    bool sbytes, cbytes, hbytes;
    size_t planeV, bytes;
};
inline GibbsWorkspace carve_gibbs(const PlanCtx* ctx, void* base, int rows, int n_vis, int n_hid, int v_pieces, int mode, bool clamp) {
    GibbsWorkspace w;
    const PlaneFormats pf = plane_formats(ctx, 3, v_pieces, mode, n_vis);
    w.hbytes = pf.hbytes;
    if (pf.gauss) { w.sp = w.cp = 3; w.sbytes = w.cbytes = false; }
    else {
        w.sp = pf.v_pieces; w.sbytes = pf.vbytes;
        if (w.sbytes) { w.cp = 1; w.cbytes = true; }
        else if (clamp) { w.cp = w.sp; w.cbytes = false; }
        else { w.cp = 1; w.cbytes = pf.nbytes; }
    }
    w.Kv = round_up(n_vis, 128); w.Kh = round_up(n_hid, 128); w.Kb = round_up(rows, 128);
    w.Lv = ld_pad(ctx, w.Kv); w.Lh = ld_pad(ctx, w.Kh);
    w.planeV = (size_t)w.Kb * w.Lv;
    Arena ar(base);
    w.v0 = ar.take<uint16_t>(w.sp * w.planeV);
    w.vc = ar.take<uint16_t>((pf.gauss ? 3 : pf.v_pieces) * w.planeV);
    w.hb = ar.take<uint16_t>((size_t)w.Kb * w.Lh);
    w.maskp = ar.take<unsigned char>((size_t)w.Kv);
    w.bytes = ar.off;
    return w;
}

// Test hook (kurbm_x3_dump_plane): where one of the planes the last complete x3 step on (rows, v_pieces, mode) left in `workspace`
// lies and how it is encoded.  fmt: 0 bf16, 1 bytes at the bf16 plane's row stride, 2 fp8 (kurbm_kernels.h: DumpArgs).
struct PlaneView { const void* src; int units, ld, fmt, transposed, pieces; size_t plane; float sign; };
inline PlaneView plane_view(const PlanCtx* ctx, const void* workspace, int which, int rows, int n_vis, int n_hid, int v_pieces, int mode) {
    const PlaneFormats pf = plane_formats(ctx, 3, v_pieces, mode, n_vis);
    const WorkspaceB w = carve_bf16(ctx, const_cast<void*>(workspace), rows, n_vis, n_hid, 3, pf.v_pieces);
    PlaneView a = {nullptr, 0, 0, 0, 0, 1, 0, 1.f};
    switch (which) {
        case KURBM_PLANE_H_POS:   a.src = w.hb;   a.units = n_hid; a.ld = w.Lh; a.fmt = pf.hbytes ? 1 : 0; break;
        case KURBM_PLANE_H_POS_T: a.src = w.hbT;  a.units = n_hid; a.ld = w.Lb; a.fmt = pf.f8pos ? 2 : 0; a.transposed = 1;
                                  if (pf.split_stats) { a.fmt = 1; a.ld = 2 * w.Lb; }
                                  break;
        case KURBM_PLANE_V_NEG:   a.src = w.v2b;  a.units = n_vis; a.ld = w.Lv; a.fmt = pf.nbytes ? 1 : 0;
                                  a.pieces = pf.vn_pieces; a.plane = w.planeV; break;
        case KURBM_PLANE_V_NEG_T: a.src = w.v2bT; a.units = n_vis; a.ld = w.Lb; a.transposed = 1;
                                  a.pieces = pf.vn_pieces; a.plane = w.planeVT;
                                  if (pf.vneg_tr) {   // (no transposed copy exists: the statistics read the row-major pieces)
                                      a.src = w.v2b; a.ld = w.Lv; a.transposed = 0; a.plane = w.planeV;
                                  }
                                  if (pf.tbytes_n) { a.fmt = 1; a.ld = 2 * w.Lb; }
                                  break;
        case KURBM_PLANE_H_NEG_T: a.src = w.hnT;  a.units = n_hid; a.ld = w.Lb; a.transposed = 1; a.pieces = 3; a.plane = w.planeHT;
                                  a.sign = -1.f; break;
        default: break;   // (units stays 0: the caller refuses it)
    }
    return a;
}

}  // namespace kurbm
#endif  // KURBM_PLAN_H
