// kurbm_host_x3.hip -- the bf16-operand paths of the C ABI (include/kurbm.h; kernels: kurbm_bf16.hip, kurbm_x3.hip): weight mirrors,
// half steps, the CD step and its stages, score, plane dump, Gibbs runs, free energy, resident data planes.
//   pieces = 1  "bf16": operands rounded to bf16 (BASELINE.json config 5)
//   pieces = 3  "x3":   every fp32 operand carried EXACTLY as three bf16 pieces (hi + mid + lo), one
//                       k-segment of the NT GEMM per pair of pieces; 0/1 samples are a single piece
// Launch sequences only: plans, plane formats and layouts are in kurbm_plan.h, the shared checks in kurbm_host.h.
#include "kurbm_host.h"

using namespace kurbm;

// segment codes of k_gemm_pb: A piece ia against B pieces 0 .. npb-1
static int pb_codes(const kurbm_ctx* ctx, int a_pieces, int b_pieces, unsigned set, unsigned long long* codes, int nseg) {
    const bool full = knob(ctx, KN_X3_FULL) != 0;
    for (int ia = 0; ia < a_pieces; ++ia) {
        int npb = b_pieces;
        if (a_pieces > 1 && b_pieces > 1 && !full) npb = b_pieces - ia;     // pairs with ia + ib <= 2
        if (npb < 1) npb = 1;
        *codes |= (unsigned long long)((unsigned)ia | ((unsigned)npb << 2) | (set << 4)) << (5 * nseg);
        ++nseg;
    }
    return nseg;
}

static inline uint32_t inv_of(int nkt) { return nkt > 1 ? (uint32_t)(0x100000000ull / (unsigned)nkt) + 1u : 0u; }

// every k_gemm_pb launch: how its blocks are mapped to tiles (two knobs), then the launch
static hipError_t launch_pb(const kurbm_ctx* ctx, int epi, GemmArgsB& g, hipStream_t st) {
    g.xcd2d = knob(ctx, KN_X3_XCD2D); g.map_force = knob(ctx, KN_MAP_SLOW); g.packed_epi = knob(ctx, KN_X3_PACKED_EPI) != 0;
    return launch_gemm_pb(epi, g, st);
}

// both weight mirrors from the fp32 master
static hipError_t launch_mirror(const kurbm_params* p, const Mirror& m, hipStream_t st) {
    return launch_f32_to_bf16(p->W, p->n_vis, p->n_hid, p->ldw, m.Wb, m.ldW, p->n_vis, m.Wtb, m.ldWt, p->n_hid, m.pieces, m.planeW,
                              m.planeWt, nullptr, 0, st);
}

// optional outputs and side products of a bf16 half step
struct HalfOutB {
    uint16_t* out = nullptr; int ldo = 0;                 // bf16 value plane, row-major
    int out_pieces = 1; size_t out_plane = 0;             // (x3, real-valued plane: its three pieces)
    int out_rows_pad = 0;                                 // rows [rows, out_rows_pad) of that plane are written as zeros
    uint16_t* outT = nullptr; int ldoT = 0;               // ... transposed
    int outT_pieces = 1; size_t outT_plane = 0;
    bool outT_neg = false;                                // the transposed plane is stored negated
    bool outT_f8 = false;                                 // the transposed plane of a 0/1 sample as fp8 bytes
    bool outT_b8 = false;                                 // ... as k-permuted bytes (0x40 = one), at the bf16 plane's row stride
    bool out_bytes = false;                               // the row-major plane of a 0/1 sample as bytes (0x40 = one)
    float* out_f32 = nullptr; float* prob_f32 = nullptr; float* out_u = nullptr; int ldo32 = 0;
    float* colpart = nullptr; int ld_colpart = 0;         // bias partials: one row per 64-row half of a 128-row tile, whatever the tile
    float colsign = 1.f;                                  // x3: colpart = colsign * column sums of the value plane
    float* rowpart = nullptr; int ld_rowpart = 0;         // x3, Bernoulli draws: softplus row sums of the tile's columns (the score)
    int* grid_n_out = nullptr;                            // ... and how many column tiles wrote them
};

// one half step: A [rows][lda] bf16 in a_pieces pieces (k padded), weights from the mirror
static int half_step_b(kurbm_ctx* ctx, int layout, const kurbm_params* p, const Mirror& m, const uint16_t* A, int lda,
                       int a_pieces, size_t a_plane, int rows, int act, int noise, const RngArgs* rng, const HalfOutB& o,
                       hipStream_t st, bool a_bytes = false) {
    GemmArgsB g;
    memset(&g, 0, sizeof g);
    const bool vh = (layout == LAYOUT_VH);
    g.A0 = A; g.lda = lda; g.a_plane0 = a_plane;
    g.B0 = vh ? m.Wtb : m.Wb; g.ldb = vh ? m.ldWt : m.ldW; g.b_plane0 = vh ? m.planeWt : m.planeW;
    // k extent: whole 64-deep k-tiles over the units (the planes and the mirror are zero-padded to 128 beyond them, so the
    // last tile reads zeros past n; 784 visibles are 13 tiles, not the 14 of the padded extent)
    g.M = rows; g.N = vh ? p->n_hid : p->n_vis; g.K = round_up(vh ? p->n_vis : p->n_hid, 64);
    // x3: one A tile against the three pieces of the weight tile (kurbm_x3.hip); rounded bf16: against its one piece
    g.nseg = pb_codes(ctx, a_pieces, m.pieces, 0u, &g.seg_codes, 0);
    g.pb_max = m.pieces;
    // a real-valued A operand: its three segments per k position, so that they can share one staging of the B pieces
    // (k_gemm_pb, "BSP"; launch_gemm_pb checks the pattern) on 128 x 128 tiles as TWO tiles per k position: the paired walk
    const bool pair = g.nseg == 3 && m.pieces == 3 && knob(ctx, KN_X3_PAIR) != 0;
    if (pair) { g.seg_fastest = 1; g.inv_nseg = inv_of(3); }
    g.pair_ok = pair ? 1 : 0;
    g.a_bytes = a_bytes ? 1 : 0;   // (a byte plane of 0/1 values: one piece, lda bytes between its rows)
    g.cfg = 0;
    // 2: 256 x 64 tiles (fewer bytes per k-tile).  Whole 256-row tiles only: the bias partial rows are laid out
    // per 64 rows, two per 128-row tile, and an even number of those is what both tilings agree on
    const int tall = knob(ctx, KN_X3_TALL);
    // (x3 only: with ONE piece per weight the B tile is the light operand and 128 x 128 tiles take fewer bytes per MFMA --
    //  A 16 KB + B 16 KB against 32 + 8 for the same 128 MFMAs per wave pair; 4096 x 4096 PCD-10, 1024 rows: 0.977 against
    //  1.033 ms per step)
    if (!pair && ceil_div(rows, 128) % 2 == 0 &&
        (tall == 1 || (tall < 0 && m.pieces == 3 && (rows / 256) * ceil_div(g.N, 64) * 4 >= 3 * ctx->plan.ncu))) g.cfg = 2;
    // (64-column tiles: a row-major plane is the next GEMM's A operand, k-padded to 128 -- cover the padded row)
    g.grid_m = ceil_div(rows, g.cfg == 2 ? 256 : 128);
    g.grid_n = g.cfg ? ceil_div(o.out ? round_up(g.N, 128) : g.N, 64) : ceil_div(g.N, 128);
    g.nkt = g.K / 64;
    g.inv_nkt = inv_of(g.nkt);
    g.kt_total = g.nseg * g.nkt; g.kt_per_split = g.kt_total; g.nsplit = 1;
    // the units end in the first k-step of the last k-tile (784 visibles: 24.5 k-steps of 32 in 13 tiles): its second k-step is padding
    // in both operands, and the byte-plane walk does not multiply it (launch_gemm_pb clears the flag for every other walk)
    g.k_tail = (knob(ctx, KN_X3_KTAIL) != 0 && round_up(vh ? p->n_vis : p->n_hid, 32) < g.K) ? 1 : 0;
    g.bias = vh ? p->b_h : p->b_v;
    g.act = act; g.noise = noise;
    if (rng) g.rng = *rng;
    g.out = o.out; g.ldo = o.ldo; g.ldo_cols = o.out ? o.ldo : g.N;
    g.out_pieces = o.out_pieces; g.out_plane = o.out_plane; g.out_bytes = o.out_bytes ? 1 : 0; g.out_rows_pad = o.out_rows_pad;
    g.outT = o.outT; g.ldoT = o.ldoT; g.outT_pieces = o.outT_pieces; g.outT_plane = o.outT_plane;
    g.outT_neg = o.outT_neg ? 1 : 0; g.outT_f8 = o.outT_b8 ? 2 : o.outT_f8 ? 1 : 0;
    g.out_f32 = o.out_f32; g.prob_f32 = o.prob_f32; g.out_u = o.out_u; g.ldo32 = o.ldo32;
    g.colpart = o.colpart; g.ld_colpart = o.ld_colpart; g.colsign = o.colsign;
    if (o.rowpart) {
        g.rowpart = o.rowpart; g.ld_rowpart = o.ld_rowpart; g.rp = 1;
        if (o.grid_n_out) *o.grid_n_out = ceil_div(g.N, g.cfg == 2 ? 64 : 128);   // (tiles in the column padding write zeros)
    }
    // row tiles fastest: an XCD's run of workgroups then shares ONE column tile, whose weight pieces
    // (the operand loaded straight into registers, one tile ahead) stay in that XCD's L2
    g.m_fastest = knob(ctx, KN_X3_MFAST);
    HIP_TRY(launch_pb(ctx, EPI_HALFSTEP, g, st));
    return KURBM_OK;
}

// mirror and workspace of an entry point that takes both: present and aligned (one refusal), then large enough
static int check_mirror_ws(const void* mirror, size_t mirror_need, size_t mirror_bytes, const void* ws, size_t ws_need, size_t ws_bytes) {
    if (!mirror || !ws || !aligned16(mirror) || !aligned16(ws)) return fail_msg(KURBM_ERR_ARG, "mirror/workspace null or misaligned");
    if (int e = check_buffer("mirror", mirror, mirror_need, mirror_bytes)) return e;
    return check_workspace(ws, ws_need, ws_bytes);
}

namespace kurbm {

int mirror_refresh_any(kurbm_ctx* ctx, int pieces, const kurbm_params* p, void* mirror, size_t mirror_bytes, kurbm_stream_t stream) {
    if (!ctx) return fail_msg(KURBM_ERR_ARG, "ctx is null");
    if (int e = check_params(p)) return e;
    const Mirror m = carve_mirror(&ctx->plan, mirror, p->n_vis, p->n_hid, pieces);
    if (int e = check_buffer("mirror", mirror, m.bytes, mirror_bytes)) return e;
    HIP_TRY(launch_mirror(p, m, static_cast<hipStream_t>(stream)));
    return KURBM_OK;
}

// Every argument check of a bf16 / x3 CD step, before anything is enqueued.  The data-parallel step runs it BEFORE its first
// collective too: a rank that fails here returns without having joined an all-reduce, and so must every other rank -- the
// checks depend only on arguments that are the same on all ranks (shapes, options, buffer sizes), except `rows`, which a rank
// may have none of (zero_rows_ok).
int check_cd_args(kurbm_ctx* ctx, int pieces, int v_pieces, const kurbm_params* p, const void* mirror, size_t mirror_bytes,
                  const float* v_batch, int rows, int ldv, const kurbm_cd_opts* o, const void* workspace,
                  size_t workspace_bytes, bool zero_rows_ok) {
    if (!ctx || !o) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_params(p)) return e;
    if (rows < 0 || (rows == 0 && !zero_rows_ok)) return fail_msg(KURBM_ERR_ARG, "rows must be positive");
    if (rows > 0)
        if (int e = check_batch(v_batch, rows, ldv, p->n_vis)) return e;
    // (a rank without rows of a remainder batch passes the clipped start of its empty shard: nothing is drawn for it)
    if (int e = check_opts(o, true, rows > 0)) return e;
    if (int e = check_v_pieces(v_pieces)) return e;
    if (o->v_chain && !aligned16(o->v_chain)) return fail_msg(KURBM_ERR_ARG, "v_chain is misaligned");
    if (o->v_planes && !aligned16(o->v_planes)) return fail_msg(KURBM_ERR_ARG, "v_planes is misaligned");
    return check_mirror_ws(mirror, carve_mirror(&ctx->plan, nullptr, p->n_vis, p->n_hid, pieces).bytes, mirror_bytes, workspace,
                           carve_bf16(&ctx->plan, nullptr, rows > 0 ? rows : 1, p->n_vis, p->n_hid, pieces, v_pieces == 3 ? 3 : 1).bytes,
                           workspace_bytes);
}

}  // namespace kurbm

static int half_step_any(kurbm_ctx* ctx, int pieces, int in_pieces, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                         int dir, const float* in, int rows, int ld_in, int act, int noise, const kurbm_rng* rng,
                         float* out_sample, float* out_prob, float* out_u, int ld_out, void* workspace,
                         size_t workspace_bytes, kurbm_stream_t stream) {
    if (!ctx) return fail_msg(KURBM_ERR_ARG, "ctx is null");
    if (int e = check_params(p)) return e;
    if (dir != 0 && dir != 1) return fail_msg(KURBM_ERR_ARG, "dir must be 0 (v->h) or 1 (h->v)");
    // x3 only: 0/1 input as the byte plane the steps keep their 0/1 data and samples in (step_chain, pf.vbytes); KURBM_X3_BYTES = 0
    // keeps it one bf16 piece, as it does there
    const bool in_binary = pieces == 3 && in_pieces == (1 | KURBM_V_BINARY);
    if (in_binary) in_pieces = 1;
    if (in_pieces != 1 && in_pieces != 3)
        return fail_msg(KURBM_ERR_ARG, pieces == 3 ? "in_pieces must be 1, 1 | KURBM_V_BINARY or 3" : "in_pieces must be 1 or 3");
    const bool in_bytes = in_binary && knob(ctx, KN_X3_BYTES) != 0;
    const int K = dir == 0 ? p->n_vis : p->n_hid, N = dir == 0 ? p->n_hid : p->n_vis;
    if (int e = check_batch(in, rows, ld_in, K, "input")) return e;
    if (noise != NOISE_NONE && (!rng || (rng->row0 & 3))) return fail_msg(KURBM_ERR_ARG, "rng missing or row0 not a multiple of 4");
    if (!out_sample && !out_prob) return fail_msg(KURBM_ERR_ARG, "both outputs are null");
    if (ld_out % 4 != 0 || ld_out < N) return fail_msg(KURBM_ERR_ARG, "ld_out %% 4 != 0 or ld_out < columns");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Mirror m = carve_mirror(&ctx->plan, mirror, p->n_vis, p->n_hid, pieces);
    // the input plane is staged at the front of the workspace, in the larger of the two row-major buffers' shapes
    const int Kp = ld_pad(&ctx->plan, round_up(K, 128)), Kb = round_up(rows, 128);   // Kp: leading dimension of the staged input
    const size_t plane = (size_t)Kb * Kp;
    // (the staged input needs less, but the contract is one size for every call on these rows: kurbm_{bf16,x3}_workspace_bytes)
    size_t need = align_up(in_pieces * plane * 2);
    const size_t query = carve_bf16(&ctx->plan, nullptr, rows, p->n_vis, p->n_hid, pieces, pieces == 3 ? in_pieces : 1).bytes;
    if (query > need) need = query;
    if (int e = check_mirror_ws(mirror, m.bytes, mirror_bytes, workspace, need, workspace_bytes)) return e;
    uint16_t* Ab = static_cast<uint16_t*>(workspace);
    HIP_TRY(launch_f32_to_bf16(in, rows, K, ld_in, Ab, Kp, Kb, nullptr, 0, 0, in_pieces, plane, 0, nullptr, 0, st, 0, in_bytes ? 1 : 0));
    RngArgs r;
    if (rng) r = make_rng(rng);
    HalfOutB o;
    o.out_f32 = (noise == NOISE_NONE) ? (out_prob ? out_prob : out_sample) : out_sample;
    o.prob_f32 = (noise == NOISE_NONE) ? nullptr : out_prob;
    o.out_u = out_u; o.ldo32 = ld_out;
    return half_step_b(ctx, dir == 0 ? LAYOUT_VH : LAYOUT_HV, p, m, Ab, Kp, in_pieces, plane, rows, act, noise,
                       rng ? &r : nullptr, o, st, in_bytes);
}

// ---- the CD step -----------------------------------------------------------------------
// One step in flight: its arguments, the formats of its planes and where they lie.  The sequence is three groups of launches --
// the chain, the statistics, the reduction with the weight mirrors -- of which cd_step_any runs all or some.
struct StepB {
    kurbm_ctx* ctx;
    int pieces;
    const kurbm_params* p;
    const kurbm_cd_opts* o;
    const float* v_batch;
    int rows, ldv, which;
    hipStream_t st;
    PlaneFormats pf;
    Mirror m;
    WorkspaceB w;
    const float* part_v_pos;   // the positive column sums of resident planes (kurbm_cd_opts::v_planes), else null
    bool need_w() const { return (which & 1) || o->delta_out; }
    int gp_v() const { return ceil_div(rows, 64); }        // 64-row bands of v_pos: rows of its column sums
    int gm() const { return ceil_div(rows, 128); }         // row tiles of the half steps (bias partial rows, in 128-row units)
};

// The chain: conversion of v_pos (stage 0), h_pos and the start of a persistent chain (1), the k - 1 inner sweeps and v_neg (2),
// h_neg (3).  stage < 0: all of them; else that one alone, on the planes a previous complete step left in the workspace.
static int step_chain(const StepB& s, int stage) {
    const kurbm_cd_opts* o = s.o;
    const kurbm_params* p = s.p;
    const WorkspaceB& w = s.w;
    const PlaneFormats& pf = s.pf;
    const auto on = [stage](int n) { return stage < 0 || stage == n; };
    const ModeActs ma = mode_acts(pf.gauss);
    const uint32_t base = o->chain * 64u;
    const int rows = s.rows;
    int e;
    // v_pos -> bf16 pieces, row-major (A of the v->h step) and transposed (statistics)
    // (x3: plus the column sums of v_pos per 64-row band, the positive half of the visible-bias statistics)
    // resident planes (kurbm_x3_convert_rows ran once for these rows): no conversion; the positive column sums stay where
    // they are and the slab reducer adds them in front of the negative ones (same order of additions either way)
    if (!o->v_planes && on(0))
        HIP_TRY(launch_f32_to_bf16(s.v_batch, rows, p->n_vis, s.ldv, w.vb, w.Lv, w.Kb, w.vbT, w.Lb, p->n_vis, pf.v_pieces, w.planeV,
                                   w.planeVT, w.part_v, w.ldv32, s.st, pf.f8pos ? 1 : 0, pf.vbytes ? 1 : 0));
    const uint16_t* h_cur = w.hb;
    // h_t ~ p(h | v) for a v that is not the data (the chain's start, the inner sweeps of CD-k): the row-major plane h2b alone
    const auto hidden_of = [&](const uint16_t* v, int v_pieces, bool v_bytes, const RngArgs& r) {
        HalfOutB ho;
        ho.out = w.h2b; ho.ldo = w.Lh; ho.out_bytes = pf.hbytes;
        h_cur = w.h2b;
        return half_step_b(s.ctx, LAYOUT_VH, p, s.m, v, w.Lv, v_pieces, w.planeV, rows, ma.act_h, NOISE_BERNOULLI, &r, ho, s.st, v_bytes);
    };
    if (on(1)) {
        // h_pos ~ p(h | v_pos)                                          rbm.py:120
        RngArgs r = make_rng(o->seed, o->row0, base + 0u, o->step);
        HalfOutB ho;
        ho.out = w.hb; ho.ldo = w.Lh; ho.out_bytes = pf.hbytes; ho.outT = w.hbT; ho.ldoT = w.Lb; ho.outT_f8 = pf.f8pos; ho.outT_b8 = pf.split_stats;
        ho.colpart = w.part_h; ho.ld_colpart = w.ldh32; ho.colsign = 1.f;
        if ((e = half_step_b(s.ctx, LAYOUT_VH, p, s.m, w.vb, w.Lv, pf.v_pieces, w.planeV, rows, ma.act_h, NOISE_BERNOULLI, &r, ho, s.st, pf.vbytes))) return e;
        if (o->v_chain) {   // persistent chain: negative phase starts from the stored fantasy particles
            HIP_TRY(launch_f32_to_bf16(o->v_chain, rows, p->n_vis, s.ldv, w.cb, w.Lv, w.Kb, nullptr, 0, 0, pf.v_pieces, w.planeV, 0, nullptr, 0, s.st,
                                       0, pf.vbytes ? 1 : 0));
            if ((e = hidden_of(w.cb, pf.v_pieces, pf.vbytes, make_rng(o->seed, o->row0, base + 32u, o->step)))) return e;
        }
    }
    for (int t = 1; on(2) && t <= o->k; ++t) {
        const bool last = (t == o->k);
        RngArgs r = make_rng(o->seed, o->row0, base + 2u * t - 1u, o->step);      // v_t ~ p(v | h_{t-1})   rbm.py:121-123
        HalfOutB ho;
        ho.out = w.v2b; ho.ldo = w.Lv; ho.out_pieces = pf.vn_pieces; ho.out_plane = w.planeV; ho.out_bytes = pf.nbytes;
        if (last) {
            if (pf.vneg_tr) ho.out_rows_pad = w.Kb;      // (the statistics walk the batch padded to 128 rows of this plane)
            else { ho.outT = w.v2bT; ho.ldoT = w.Lb; ho.outT_pieces = pf.vn_pieces; ho.outT_plane = w.planeVT; ho.outT_b8 = pf.tbytes_n; }
            ho.out_f32 = o->v_chain; ho.ldo32 = s.ldv;
            // -sum(v_neg) below the bands of +sum(v_pos); nothing for the inner steps of CD-k
            ho.colpart = w.part_v + (size_t)s.gp_v() * w.ldv32;
        }
        ho.ld_colpart = w.ldv32; ho.colsign = -1.f;
        if ((e = half_step_b(s.ctx, LAYOUT_HV, p, s.m, h_cur, w.Lh, 1, 0, rows, ma.act_v, ma.noise_v, &r, ho, s.st, pf.hbytes))) return e;
        if (!last && (e = hidden_of(w.v2b, pf.vn_pieces, pf.nbytes, make_rng(o->seed, o->row0, base + 2u * t, o->step)))) return e;
    }
    // h_neg = sigmoid(v_neg.W + b_h), probabilities (rbm.py:124): only its transposed image is needed, and only by the
    // statistics GEMM, where it enters with a minus sign: it is stored as -h_neg
    if (on(3)) {
        HalfOutB ho;
        ho.outT = w.hnT; ho.ldoT = w.Lb; ho.outT_pieces = s.pieces; ho.outT_plane = w.planeHT; ho.outT_neg = true;
        ho.colpart = w.part_h + (size_t)2 * s.gm() * w.ldh32; ho.ld_colpart = w.ldh32; ho.colsign = -1.f;
        if ((e = half_step_b(s.ctx, LAYOUT_VH, p, s.m, w.v2b, w.Lv, pf.vn_pieces, w.planeV, rows, ACT_SIGMOID, NOISE_NONE, nullptr, ho, s.st, pf.nbytes))) return e;
    }
    return KURBM_OK;
}

// One launch of the statistics: what plan `q` and the step fix of its arguments (g: operands, segments and walk set by the caller)
static int stats_gemm(const StepB& s, GemmArgsB& g, const OuterPlan& q, int M, int N, float* slab, size_t slab_stride) {
    g.M = M; g.N = N; g.K = s.w.Kb;
    g.grid_m = q.gm; g.grid_n = q.gn; g.cfg = q.cfg;
    g.slab = slab; g.slab_stride = slab_stride; g.ld_slab = q.ld_slab;
    g.m_fastest = knob(s.ctx, KN_X3_STATS_MFAST);
    g.nkt = q.nkt; g.inv_nkt = inv_of(g.nkt);
    g.kt_total = q.kt_total; g.kt_per_split = q.kt_per_split; g.nsplit = q.nsplit;
    HIP_TRY(launch_pb(s.ctx, EPI_SLAB, g, s.st));
    return KURBM_OK;
}

// The statistics of visible rows [m_lo, m_lo + Mr): dW = v_pos^T.h_pos - v_neg^T.h_neg as split-K slabs -- NT GEMMs over the
// transposed images, k = batch
static int step_statistics(const StepB& s, const StatsPlan& sp, int m_lo, int Mr) {
    const WorkspaceB& w = s.w;
    const PlaneFormats& pf = s.pf;
    const int n_hid = s.p->n_hid;
    GemmArgsB g;
    memset(&g, 0, sizeof g);
    if (!pf.split_stats) {
        g.A0 = w.vbT + (size_t)m_lo * w.Lb; g.a_plane0 = w.planeVT; g.B0 = w.hbT;
        g.A1 = w.v2bT + (size_t)m_lo * w.Lb; g.a_plane1 = w.planeVT; g.B1 = w.hnT; g.b_plane1 = w.planeHT;
        g.lda = w.Lb; g.ldb = w.Lb;
        if (pf.tbytes) { g.a_bytes = 1; g.lda = 2 * w.Lb; }   // (both A planes hold one byte per element at the bf16 planes' row stride)
        // (piece of v_pos) x h_pos, then v_neg x (all pieces of h_neg), walked segment-fastest
        g.nseg = pb_codes(s.ctx, pf.v_pieces, 1, 0u, &g.seg_codes, 0);
        g.nseg = pb_codes(s.ctx, pf.vn_pieces, s.pieces, 1u, &g.seg_codes, g.nseg);
        g.pb_max = s.pieces;
        g.seg_fastest = 1; g.inv_nseg = inv_of(g.nseg);
        if (pf.f8pos) { g.f8pos = 1; g.inv_nseg = inv_of(2 * g.nseg - 1); }   // (tiles per 128-deep unit)
        return stats_gemm(s, g, sp.pl, Mr, n_hid, w.slab, sp.slab_stride);
    }
    // ---- negative half: slabs [0, neg.nsplit)
    g.A0 = w.v2bT + (size_t)m_lo * w.Lb; g.a_plane0 = w.planeVT; g.B0 = w.hnT; g.b_plane0 = w.planeHT;
    g.lda = w.Lb; g.ldb = w.Lb;
    g.pb_max = 3;
    if (pf.gauss) {   // (v_neg piece a) x (-h_neg pieces 0 .. 2 - a), two tiles per k position (k_gemm_pb, "BSP")
        g.nseg = pb_codes(s.ctx, 3, 3, 0u, &g.seg_codes, 0);
        g.seg_fastest = 1; g.inv_nseg = inv_of(g.nseg); g.pair_ok = 1;
        if (pf.vneg_tr) {   // A = the ROW-MAJOR pieces [batch][n_vis]: columns m_lo .. of them
            g.A0 = w.v2b + m_lo; g.a_plane0 = w.planeV; g.lda = w.Lv; g.a_tr = 1;
        }
    } else {       // v_neg^T as bytes against the three pieces of -h_neg^T (k_gemm_pb, "ABP")
        g.nseg = pb_codes(s.ctx, 1, 3, 0u, &g.seg_codes, 0);
        g.a_bytes = 1; g.lda = 2 * w.Lb;
    }
    if (int e = stats_gemm(s, g, sp.sps.neg, Mr, n_hid, w.slab, sp.slab_stride)) return e;
    // ---- positive half, transposed: h_pos^T (bytes) x the pieces of v_pos^T -> slabs [neg.nsplit, +pos.nsplit)
    memset(&g, 0, sizeof g);
    g.A0 = w.hbT; g.a_bytes = 1; g.lda = 2 * w.Lb;
    g.B0 = w.vbT + (size_t)m_lo * w.Lb; g.b_plane0 = w.planeVT; g.ldb = w.Lb;
    g.slab_t = 1;
    g.pb_max = 3;
    g.nseg = pb_codes(s.ctx, 1, 3, 0u, &g.seg_codes, 0);
    return stats_gemm(s, g, sp.sps.pos, n_hid, Mr, w.slab + (size_t)sp.sps.neg.nsplit * sp.slab_stride, sp.slab_stride);
}

// The tail: slabs and bias partials reduced, lr * sums applied (rbm.py:127-134) and / or the packed delta emitted, and the weight
// mirrors brought up to date.  reduce = false (stage 6): the mirror refresh alone.
static int step_reduce(const StepB& s, const StatsPlan& sp, int m_lo, int m_hi, const kurbm_momentum* mom, bool reduce) {
    const kurbm_params* p = s.p;
    const WorkspaceB& w = s.w;
    const int Mr = m_hi - m_lo, gp_v = s.gp_v(), gm = s.gm();
    const bool sub = (Mr != p->n_vis);
    ReduceArgs a;
    memset(&a, 0, sizeof a);
    a.slab = w.slab; a.slab_stride = sp.slab_stride; a.ld_slab = sp.pl.ld_slab;
    a.nslab = s.pf.split_stats ? sp.sps.neg.nsplit + sp.sps.pos.nsplit : sp.pl.nsplit;
    a.n_vis = Mr; a.n_hid = p->n_hid; a.ldw = p->ldw;
    a.nblk_w = s.need_w() ? (int)(((long long)Mr * (sp.pl.ld_slab / 4) + 255) / 256) : 0;
    reduce_targets(a, p, s.o, s.which, m_lo);
    a.part_h = w.part_h; a.nrow_tiles_h = 4 * gm; a.ld_part_h = w.ldh32;
    a.part_v = w.part_v; a.nrow_tiles_v = gp_v + 2 * gm; a.ld_part_v = w.ldv32;
    if (s.part_v_pos) {   // rows [0, gp_v) from the resident planes, then the workspace's negative rows
        a.part_v = s.part_v_pos; a.nrow_tiles_v = gp_v;
        a.part_v2 = w.part_v + (size_t)gp_v * w.ldv32; a.nrow_tiles_v2 = 2 * gm;
    }
    if (sub && m_hi != p->n_vis) { a.part_h = nullptr; a.part_v = nullptr; a.part_v2 = nullptr; }   // the bias sums leave with the LAST rows
    if (sub) a.n_vis_bias = p->n_vis;
    // the fp32 master moves: the slab reduction writes the new weights AND their bf16 pieces in one pass
    // (the velocity rows of an n_hid that is no multiple of 4 are not 16-byte aligned: the two-launch form serves them)
    const bool mirror_in_reduce = a.W && s.need_w() && !knob(s.ctx, KN_UNFUSED_MIRROR) && !(mom && (p->n_hid & 3));
    if (mirror_in_reduce) {
        a.Wb = s.m.Wb; a.ldWb = s.m.ldW; a.planeWb = s.m.planeW;
        a.Wtb = s.m.Wtb; a.ldWtb = s.m.ldWt; a.planeWtb = s.m.planeWt; a.pieces = s.pieces;
        a.tile_rows = knob(s.ctx, KN_REDUCE_TR);
    }
    const MomOpt mo = make_mom(p, mom);
    if (reduce) HIP_TRY(mirror_in_reduce ? launch_reduce_apply_split(a, s.st, nullptr, mo.ptr()) : launch_reduce_apply(a, s.st, mo.ptr()));
    // two launches, or the refresh alone: the fp32 master moved (will have moved), re-derive both mirrors
    if (mirror_in_reduce ? !reduce : a.W != nullptr) HIP_TRY(launch_mirror(p, s.m, s.st));
    return KURBM_OK;
}

namespace kurbm {

// mom (nullable; whole steps only): the update goes through the velocity, in the same launch (kurbm_cd_step_x3_mom, _bf16_mom).
// `only` 0..6 (measurement hook kurbm_cd_step_x3_stage): launch just that stage of the sequence, on the planes a previous complete
// step left in the workspace -- 0..3 of the chain, 4 the statistics, 5 the reduction, 6 the mirror refresh.  8: the chain alone
// (kurbm_cd_chain_x3).  7: the statistics and reduction of visible rows [m_lo, m_hi) alone (kurbm_x3_stats_rows) -- the
// data-parallel step all-reduces the first rows of dW while the rest is still being computed.
int cd_step_any(kurbm_ctx* ctx, int pieces, int v_pieces, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                const float* v_batch, int rows, int ldv, const kurbm_cd_opts* o, int which, void* workspace,
                size_t workspace_bytes, kurbm_stream_t stream, int only, int m_lo, int m_hi, const kurbm_momentum* mom) {
    if (int e = check_cd_args(ctx, pieces, v_pieces, p, mirror, mirror_bytes, v_batch, rows, ldv, o, workspace, workspace_bytes, false)) return e;
    if (mom) {
        if (int e = check_mom(mom, o)) return e;
        if (only >= 0) return fail_msg(KURBM_ERR_ARG, "momentum applies to whole steps only");
    }
    if (m_hi < 0) m_hi = p->n_vis;
    const PlanCtx* pc = &ctx->plan;
    StepB s = {ctx, pieces, p, o, v_batch, rows, ldv, which, static_cast<hipStream_t>(stream),
               plane_formats(pc, pieces, v_pieces, o->mode, p->n_vis), carve_mirror(pc, mirror, p->n_vis, p->n_hid, pieces), {}, nullptr};
    s.w = carve_bf16(pc, workspace, rows, p->n_vis, p->n_hid, pieces, s.pf.v_pieces);
    if (o->v_planes) {
        const VPlanes vp = carve_vplanes(pc, o->v_planes, rows, p->n_vis, s.pf.v_pieces);
        s.w.vb = vp.vb; s.w.vbT = vp.vbT; s.part_v_pos = vp.part_v;
    }
    const StatsPlan sp = plan_stats(pc, pieces, v_pieces, o->mode, rows, p->n_vis, p->n_hid, m_lo, m_hi);
    const bool all = only < 0;
    if (all || only <= 3 || only == 8)
        if (int e = step_chain(s, (all || only == 8) ? -1 : only)) return e;
    if (s.need_w() && (all || only == 4 || only == 7))
        if (int e = step_statistics(s, sp, m_lo, m_hi - m_lo)) return e;
    if (all || (only >= 5 && only <= 7)) return step_reduce(s, sp, m_lo, m_hi, mom, only != 6);
    return KURBM_OK;
}

// W (rows [m_lo, m_hi)), and with `bias` b_h and b_v, += lr * (packed delta); the bf16 pieces of the new weights rewritten
// in both orientations -- one launch: the packed delta is one "slab" and one row of bias partials each.
int apply_delta_rows(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, int pieces, const float* delta,
                     float lr, int which, int m_lo, int m_hi, bool bias, hipStream_t st, const kurbm_momentum* mom) {
    const Mirror m = carve_mirror(&ctx->plan, mirror, p->n_vis, p->n_hid, pieces);
    if (m.bytes > mirror_bytes) return fail_msg(KURBM_ERR_WORKSPACE, "mirror too small: need %zu bytes, got %zu", m.bytes, mirror_bytes);
    ReduceArgs a;
    memset(&a, 0, sizeof a);
    const size_t nw = (size_t)p->n_vis * p->n_hid;
    a.slab = delta + (size_t)m_lo * p->n_hid; a.slab_stride = 0; a.nslab = 1; a.ld_slab = p->n_hid;
    a.n_vis = m_hi - m_lo; a.n_vis_bias = p->n_vis; a.n_hid = p->n_hid; a.ldw = p->ldw; a.lr = lr;
    a.W = p->W + (size_t)m_lo * p->ldw;
    if (bias) {
        a.part_h = delta + nw; a.nrow_tiles_h = 1; a.ld_part_h = p->n_hid; a.b_h = (which & 2) ? p->b_h : nullptr;
        a.part_v = delta + nw + p->n_hid; a.nrow_tiles_v = 1; a.ld_part_v = p->n_vis; a.b_v = (which & 4) ? p->b_v : nullptr;
    }
    a.Wb = m.Wb + (size_t)m_lo * m.ldW; a.ldWb = m.ldW; a.planeWb = m.planeW;
    a.Wtb = m.Wtb + m_lo; a.ldWtb = m.ldWt; a.planeWtb = m.planeWt; a.pieces = pieces;
    // the transposed mirror's k columns of these rows; the last range also rewrites the zero k padding behind n_vis
    a.wtb_k_ext = (m_hi == p->n_vis) ? m.ldWt - m_lo : m_hi - m_lo;
    a.tile_rows = knob(ctx, KN_REDUCE_TR);
    HIP_TRY(launch_reduce_apply_split(a, st, nullptr, make_mom(p, mom, m_lo).ptr()));
    return KURBM_OK;
}

}  // namespace kurbm

static int cd_epoch_x3_any(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* V,
                           int v_pieces, int n_rows, int ldv, int batch_size, const kurbm_cd_opts* opts, void* workspace,
                           size_t workspace_bytes, kurbm_stream_t stream, const kurbm_momentum* mom) {
    if (int e = check_epoch(ctx, opts, n_rows, batch_size)) return e;
    if (opts->delta_out || !opts->apply) return fail_msg(KURBM_ERR_ARG, "kurbm_cd_epoch_x3 applies in place: apply = 1, delta_out = null");
    if (opts->v_planes && opts->v_planes_stride < carve_vplanes(&ctx->plan, nullptr, batch_size < n_rows ? batch_size : (n_rows > 0 ? n_rows : 1),
                                                                 p ? p->n_vis : 1, v_pieces == 3 ? 3 : 1).bytes)
        return fail_msg(KURBM_ERR_ARG, "v_planes_stride is smaller than the planes of one batch");
    kurbm_cd_opts o = *opts;
    return for_each_batch(n_rows, batch_size, [&](int lo, int rows, int step) {
        if (opts->v_planes) o.v_planes = static_cast<const char*>(opts->v_planes) + (size_t)step * opts->v_planes_stride;
        const int e = cd_step_any(ctx, 3, v_pieces, p, mirror, mirror_bytes, V + (size_t)lo * ldv, rows, ldv, &o, 7, workspace,
                                  workspace_bytes, stream, -1, 0, -1, mom);
        ++o.step;
        return e;
    });
}

static int x3_apply_delta_any(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* delta,
                              float lr, int which, kurbm_stream_t stream, const kurbm_momentum* mom) {
    if (!ctx || !delta) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_params(p)) return e;
    if (!mirror || !aligned16(mirror) || !aligned16(delta)) return fail_msg(KURBM_ERR_ARG, "mirror / delta null or misaligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((p->n_hid & 3) || !(which & 1)) {   // packed rows not 16-byte aligned, or W untouched: two launches
        const Mirror m = carve_mirror(&ctx->plan, mirror, p->n_vis, p->n_hid, 3);
        if (int e = check_buffer("mirror", mirror, m.bytes, mirror_bytes)) return e;
        if (int e = apply_delta_f32(ctx, p, delta, lr, which, stream, mom)) return e;
        if (which & 1) HIP_TRY(launch_mirror(p, m, st));
        return KURBM_OK;
    }
    return apply_delta_rows(ctx, p, mirror, mirror_bytes, 3, delta, lr, which, 0, p->n_vis, true, st, mom);
}

static bool gibbs_shape_ok(int n_chains, int v_pieces, int mode) {
    return n_chains > 0 && (v_pieces == 1 || v_pieces == 3 || v_pieces == (1 | KURBM_V_BINARY)) &&
           (mode == KURBM_MODE_VISIBLE_BERNOULLI || mode == KURBM_MODE_VISIBLE_GAUSSIAN);
}

extern "C" {

// ---- Gibbs runs (include/kurbm.h: kurbm_gibbs_run; the workspace and its formats: kurbm_plan.h, carve_gibbs) -------------------
size_t kurbm_gibbs_workspace_bytes(kurbm_ctx* ctx, int n_chains, int n_vis, int n_hid, int v_pieces, int mode) {
    if (!ctx || n_vis <= 0 || n_hid <= 0 || !gibbs_shape_ok(n_chains, v_pieces, mode)) return 0;
    return carve_gibbs(&ctx->plan, nullptr, n_chains, n_vis, n_hid, v_pieces, mode, false).bytes;
}

// n_labels > 0: the last n_labels visible units are a FREE label block (kurbm_gibbs_run_labels): the label site rewrites the block of
// every v_t behind the h -> v launch, and the label columns of `clamp` are not read (the mask is made of the pixels alone)
static int gibbs_run_any(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, void* mirror, size_t mirror_bytes, const float* v_init,
                         int v_pieces, int ldv, int n_chains, uint64_t chain0, uint64_t seed, int mode, int burn_in, int thin, int n_keep,
                         const uint8_t* clamp, float* v_out, float* prob_out, int ldo, size_t keep_stride, void* ws, size_t ws_bytes,
                         kurbm_stream_t stream) {
    // every check before the first launch: a refused call has written nothing
    if (!ctx) return fail_msg(KURBM_ERR_ARG, "ctx is null");
    if (int e = check_params(p)) return e;
    if (n_labels) {
        if (int e = check_labels(p, n_labels)) return e;
        if (mode != KURBM_MODE_VISIBLE_BERNOULLI) return fail_msg(KURBM_ERR_ARG, "a label RBM has Bernoulli visibles");
    }
    const int n_pix = p->n_vis - n_labels;
    if (n_chains <= 0) return fail_msg(KURBM_ERR_ARG, "n_chains must be positive");
    if (int e = check_mode(mode)) return e;
    if (int e = check_v_pieces(v_pieces)) return e;
    if (burn_in < 1 || thin < 1 || n_keep < 1) return fail_msg(KURBM_ERR_ARG, "burn_in, thin and n_keep must be >= 1");
    const long long T = (long long)burn_in + (long long)(n_keep - 1) * thin;
    if (T > 0x7FFFFFFFll) return fail_msg(KURBM_ERR_ARG, "burn_in + (n_keep - 1) * thin exceeds 2^31 - 1 sweeps");
    if (chain0 & 3) return fail_msg(KURBM_ERR_ARG, "chain0 must be a multiple of 4");
    if (int e = check_batch(v_init, n_chains, ldv, p->n_vis, "v_init")) return e;
    if (int e = check_batch(v_out, n_chains, ldo, p->n_vis, "v_out")) return e;
    if (prob_out && !aligned16(prob_out)) return fail_msg(KURBM_ERR_ARG, "prob_out is misaligned");
    if (n_keep > 1 && (keep_stride < (size_t)n_chains * (size_t)ldo || keep_stride % 4 != 0))
        return fail_msg(KURBM_ERR_ARG, "keep_stride below n_chains * ldo floats, or not a multiple of 4");
    const Mirror m = carve_mirror(&ctx->plan, mirror, p->n_vis, p->n_hid, 3);
    const GibbsWorkspace w = carve_gibbs(&ctx->plan, ws, n_chains, p->n_vis, p->n_hid, v_pieces, mode, clamp != nullptr);
    if (int e = check_mirror_ws(mirror, m.bytes, mirror_bytes, ws, w.bytes, ws_bytes)) return e;     // (w.bytes: the same with or without a mask)
    if (clamp && ((size_t)w.Lv * (w.cbytes ? 1 : 2)) % 16 != 0)
        return fail_msg(KURBM_ERR_UNSUPPORTED, "clamping needs plane rows of whole 16-byte groups (KURBM_LDPAD = %d)", knob(ctx, KN_LDPAD));

    hipStream_t st = static_cast<hipStream_t>(stream);
    const auto [act_h, act_v, noise_v] = mode_acts(mode == KURBM_MODE_VISIBLE_GAUSSIAN);
    // the start plane, converted once; with a mask, the current plane starts as its copy (same format) so that every sweep reads vc
    HIP_TRY(launch_f32_to_bf16(v_init, n_chains, p->n_vis, ldv, w.v0, w.Lv, w.Kb, nullptr, 0, 0, w.sp, w.planeV, 0, nullptr, 0, st,
                               0, w.sbytes ? 1 : 0));
    if (clamp) HIP_TRY(launch_gibbs_mask(clamp, n_pix, w.maskp, w.Kv, w.cbytes ? 1 : 0, st));
    int e;
    for (long long t = 1; t <= T; ++t) {
        const bool first = t == 1;
        const long long since = t - burn_in;
        const bool kept = since >= 0 && since % thin == 0;
        const size_t joff = kept ? (size_t)(since / thin) * keep_stride : 0;
        RngArgs r = make_rng(seed, chain0, KURBM_STREAM_GIBBS_H, (uint32_t)t);          // h_t ~ p(h | v_{t-1})
        {
            HalfOutB ho;
            ho.out = w.hb; ho.ldo = w.Lh; ho.out_bytes = w.hbytes;
            if ((e = half_step_b(ctx, LAYOUT_VH, p, m, first ? w.v0 : w.vc, w.Lv, first ? w.sp : w.cp, w.planeV, n_chains, act_h,
                                 NOISE_BERNOULLI, &r, ho, st, first ? w.sbytes : w.cbytes)))
                return e;
        }
        r = make_rng(seed, chain0, KURBM_STREAM_GIBBS_V, (uint32_t)t);                  // v_t ~ p(v | h_t)
        {
            HalfOutB ho;
            ho.out = w.vc; ho.ldo = w.Lv; ho.out_pieces = w.cp; ho.out_plane = w.planeV; ho.out_bytes = w.cbytes;
            if (kept) { ho.out_f32 = v_out + joff; ho.prob_f32 = prob_out ? prob_out + joff : nullptr; ho.ldo32 = ldo; }
            if ((e = half_step_b(ctx, LAYOUT_HV, p, m, w.hb, w.Lh, 1, 0, n_chains, act_v, noise_v, &r, ho, st, w.hbytes))) return e;
        }
        if (n_labels) {   // the block of v_t: one draw of softmax(b_v + h_t.W^T), in the plane's format (and the fp32 planes of a kept sweep)
            LabelSiteArgs a;
            memset(static_cast<void*>(&a), 0, sizeof a);
            a.h = w.hb; a.ldh = w.Lh; a.hfmt = w.hbytes ? LS_H_BYTES : LS_H_BF16;
            a.W = p->W; a.ldw = p->ldw; a.b_v = p->b_v;
            if (w.cbytes) { a.vb = reinterpret_cast<unsigned char*>(w.vc); a.ldvb = (size_t)w.Lv; }
            else { a.vp = w.vc; a.ldvp = w.Lv; a.pieces = w.cp; a.plane = w.planeV; }
            if (kept) { a.v = v_out + joff; a.ldv = ldo; a.prob = prob_out ? prob_out + joff : nullptr; a.ldp = ldo; a.prob_col0 = n_pix; }
            a.rows = n_chains; a.n_pix = n_pix; a.C = n_labels; a.n_hid = p->n_hid;
            a.rng = r;
            HIP_TRY(launch_label_site(a, st));
        }
        if (clamp) {   // v_t[:, c] = v_init[:, c]: the plane the next sweep reads and, on a kept sweep, the fp32 planes just written
            GibbsClampArgs a;
            memset(static_cast<void*>(&a), 0, sizeof a);
            a.cur = reinterpret_cast<unsigned char*>(w.vc); a.start = reinterpret_cast<const unsigned char*>(w.v0); a.maskp = w.maskp;
            a.rows = n_chains; a.ngroups = w.Kv / 8; a.es = w.cbytes ? 1 : 2; a.pieces = w.cp; a.perm = w.cbytes ? 1 : 0;
            a.n_vis = p->n_vis;
            a.ld_bytes = (size_t)w.Lv * a.es; a.plane_bytes = w.planeV * 2;
            if (kept) { a.v_init = v_init; a.ldv = ldv; a.v_out = v_out + joff; a.prob_out = prob_out ? prob_out + joff : nullptr; a.ldo = ldo; }
            HIP_TRY(launch_gibbs_clamp(a, st));
        }
    }
    return KURBM_OK;
}

int kurbm_gibbs_run(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v_init, int v_pieces,
                    int ldv, int n_chains, uint64_t chain0, uint64_t seed, int mode, int burn_in, int thin, int n_keep,
                    const uint8_t* clamp, float* v_out, float* prob_out, int ldo, size_t keep_stride, void* ws, size_t ws_bytes,
                    kurbm_stream_t stream) {
    return gibbs_run_any(ctx, p, 0, mirror, mirror_bytes, v_init, v_pieces, ldv, n_chains, chain0, seed, mode, burn_in, thin, n_keep,
                         clamp, v_out, prob_out, ldo, keep_stride, ws, ws_bytes, stream);
}

int kurbm_gibbs_run_labels(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, void* mirror, size_t mirror_bytes, const float* v_init,
                           int v_pieces, int ldv, int n_chains, uint64_t chain0, uint64_t seed, int mode, int burn_in, int thin,
                           int n_keep, const uint8_t* clamp, float* v_out, float* prob_out, int ldo, size_t keep_stride, void* ws,
                           size_t ws_bytes, kurbm_stream_t stream) {
    if (!ctx) return fail_msg(KURBM_ERR_ARG, "ctx is null");
    if (int e = check_params(p)) return e;
    if (int e = check_labels(p, n_labels)) return e;     // (n_labels = 0 is the plain run's, not a label run)
    return gibbs_run_any(ctx, p, n_labels, mirror, mirror_bytes, v_init, v_pieces, ldv, n_chains, chain0, seed, mode, burn_in, thin,
                         n_keep, clamp, v_out, prob_out, ldo, keep_stride, ws, ws_bytes, stream);
}

// ---- mirrors, workspaces, half steps, steps ----------------------------------------------------------------------------------
size_t kurbm_bf16_mirror_bytes(kurbm_ctx* ctx, int n_vis, int n_hid) {
    if (!ctx || n_vis <= 0 || n_hid <= 0) return 0;
    return carve_mirror(&ctx->plan, nullptr, n_vis, n_hid, 1).bytes;
}
size_t kurbm_x3_mirror_bytes(kurbm_ctx* ctx, int n_vis, int n_hid) {
    if (!ctx || n_vis <= 0 || n_hid <= 0) return 0;
    return carve_mirror(&ctx->plan, nullptr, n_vis, n_hid, 3).bytes;
}

int kurbm_bf16_mirror_refresh(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, kurbm_stream_t stream) {
    return mirror_refresh_any(ctx, 1, p, mirror, mirror_bytes, stream);
}
int kurbm_x3_mirror_refresh(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, kurbm_stream_t stream) {
    return mirror_refresh_any(ctx, 3, p, mirror, mirror_bytes, stream);
}

size_t kurbm_bf16_workspace_bytes(kurbm_ctx* ctx, int rows, int n_vis, int n_hid, int k) {
    (void)k;
    if (!ctx || rows <= 0 || n_vis <= 0 || n_hid <= 0) return 0;
    return carve_bf16(&ctx->plan, nullptr, rows, n_vis, n_hid, 1, 1).bytes;
}
size_t kurbm_x3_workspace_bytes(kurbm_ctx* ctx, int rows, int n_vis, int n_hid, int k, int v_pieces) {
    (void)k;
    if (v_pieces == (1 | KURBM_V_BINARY)) v_pieces = 1;
    if (!ctx || rows <= 0 || n_vis <= 0 || n_hid <= 0 || (v_pieces != 1 && v_pieces != 3)) return 0;
    return carve_bf16(&ctx->plan, nullptr, rows, n_vis, n_hid, 3, v_pieces).bytes;
}

int kurbm_half_step_bf16(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, int dir,
                         const float* in, int rows, int ld_in, int act, int noise, const kurbm_rng* rng,
                         float* out_sample, float* out_prob, float* out_u, int ld_out, void* workspace,
                         size_t workspace_bytes, kurbm_stream_t stream) {
    return half_step_any(ctx, 1, 1, p, mirror, mirror_bytes, dir, in, rows, ld_in, act, noise, rng, out_sample, out_prob,
                         out_u, ld_out, workspace, workspace_bytes, stream);
}
int kurbm_half_step_x3(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, int dir,
                       const float* in, int in_pieces, int rows, int ld_in, int act, int noise, const kurbm_rng* rng,
                       float* out_sample, float* out_prob, float* out_u, int ld_out, void* workspace,
                       size_t workspace_bytes, kurbm_stream_t stream) {
    return half_step_any(ctx, 3, in_pieces, p, mirror, mirror_bytes, dir, in, rows, ld_in, act, noise, rng, out_sample,
                         out_prob, out_u, ld_out, workspace, workspace_bytes, stream);
}

int kurbm_cd_step_bf16(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v_batch,
                       int rows, int ldv, const kurbm_cd_opts* o, int which, void* workspace, size_t workspace_bytes,
                       kurbm_stream_t stream) {
    return cd_step_any(ctx, 1, 1, p, mirror, mirror_bytes, v_batch, rows, ldv, o, which, workspace, workspace_bytes, stream);
}
int kurbm_cd_step_x3(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v_batch,
                     int v_pieces, int rows, int ldv, const kurbm_cd_opts* o, int which, void* workspace,
                     size_t workspace_bytes, kurbm_stream_t stream) {
    return cd_step_any(ctx, 3, v_pieces, p, mirror, mirror_bytes, v_batch, rows, ldv, o, which, workspace, workspace_bytes, stream);
}

int kurbm_cd_step_bf16_mom(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v_batch,
                           int rows, int ldv, const kurbm_cd_opts* o, int which, void* workspace, size_t workspace_bytes,
                           kurbm_stream_t stream, const kurbm_momentum* mom) {
    if (!mom) return fail_msg(KURBM_ERR_ARG, "momentum block or its velocity buffer is null");
    return cd_step_any(ctx, 1, 1, p, mirror, mirror_bytes, v_batch, rows, ldv, o, which, workspace, workspace_bytes, stream, -1, 0, -1, mom);
}
int kurbm_cd_step_x3_mom(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v_batch,
                         int v_pieces, int rows, int ldv, const kurbm_cd_opts* o, int which, void* workspace,
                         size_t workspace_bytes, kurbm_stream_t stream, const kurbm_momentum* mom) {
    if (!mom) return fail_msg(KURBM_ERR_ARG, "momentum block or its velocity buffer is null");
    return cd_step_any(ctx, 3, v_pieces, p, mirror, mirror_bytes, v_batch, rows, ldv, o, which, workspace, workspace_bytes, stream, -1, 0, -1,
                       mom);
}

int kurbm_cd_step_x3_stage(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v_batch,
                           int v_pieces, int rows, int ldv, const kurbm_cd_opts* o, int which, int stage, void* workspace,
                           size_t workspace_bytes, kurbm_stream_t stream) {
    if (stage < 0 || stage > 6) return fail_msg(KURBM_ERR_ARG, "stage must be in [0, 6]");
    return cd_step_any(ctx, 3, v_pieces, p, mirror, mirror_bytes, v_batch, rows, ldv, o, which, workspace, workspace_bytes, stream,
                       stage);
}

int kurbm_cd_epoch_x3(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* V,
                      int v_pieces, int n_rows, int ldv, int batch_size, const kurbm_cd_opts* opts, void* workspace,
                      size_t workspace_bytes, kurbm_stream_t stream) {
    return cd_epoch_x3_any(ctx, p, mirror, mirror_bytes, V, v_pieces, n_rows, ldv, batch_size, opts, workspace, workspace_bytes, stream, nullptr);
}

int kurbm_cd_epoch_x3_mom(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* V,
                          int v_pieces, int n_rows, int ldv, int batch_size, const kurbm_cd_opts* opts, void* workspace,
                          size_t workspace_bytes, kurbm_stream_t stream, const kurbm_momentum* mom) {
    if (!opts) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_mom(mom, opts)) return e;
    return cd_epoch_x3_any(ctx, p, mirror, mirror_bytes, V, v_pieces, n_rows, ldv, batch_size, opts, workspace, workspace_bytes, stream, mom);
}

int kurbm_cd_chain_x3(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v_batch,
                      int v_pieces, int rows, int ldv, const kurbm_cd_opts* o, void* workspace, size_t workspace_bytes,
                      kurbm_stream_t stream) {
    return cd_step_any(ctx, 3, v_pieces, p, mirror, mirror_bytes, v_batch, rows, ldv, o, 7, workspace, workspace_bytes, stream, 8);
}

int kurbm_x3_stats_rows(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v_batch,
                        int v_pieces, int rows, int ldv, const kurbm_cd_opts* o, int m_lo, int m_hi, void* workspace,
                        size_t workspace_bytes, kurbm_stream_t stream) {
    if (!p || !o) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (o->apply || !o->delta_out) return fail_msg(KURBM_ERR_ARG, "kurbm_x3_stats_rows emits sums: apply = 0, delta_out set");
    if (m_lo < 0 || m_hi > p->n_vis || m_lo >= m_hi || (m_lo & 127))
        return fail_msg(KURBM_ERR_ARG, "row range: 0 <= m_lo < m_hi <= n_vis, m_lo a multiple of 128");
    return cd_step_any(ctx, 3, v_pieces, p, mirror, mirror_bytes, v_batch, rows, ldv, o, 7, workspace, workspace_bytes, stream, 7,
                       m_lo, m_hi);
}

int kurbm_free_energy_x3(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v, int v_pieces,
                         int rows, int ldv, float* F, void* workspace, size_t workspace_bytes, kurbm_stream_t stream) {
    if (!ctx || !F) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_params(p)) return e;
    if (rows <= 0) return fail_msg(KURBM_ERR_ARG, "rows must be positive");
    if (int e = check_v_pieces(v_pieces)) return e;
    if (v_pieces != 3) v_pieces = 1;
    if (int e = check_batch(v, rows, ldv, p->n_vis, "v")) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Mirror m = carve_mirror(&ctx->plan, mirror, p->n_vis, p->n_hid, 3);
    const FeX3Workspace w = carve_fe_x3(&ctx->plan, workspace, rows, p->n_vis, p->n_hid, v_pieces);
    if (int e = check_mirror_ws(mirror, m.bytes, mirror_bytes, workspace, w.bytes, workspace_bytes)) return e;
    HIP_TRY(launch_f32_to_bf16(v, rows, p->n_vis, ldv, w.Ab, w.Lp, w.Kb, nullptr, 0, 0, v_pieces, w.plane, 0, nullptr, 0, st));
    GemmArgsB g;
    memset(&g, 0, sizeof g);
    g.grid_m = w.grid_m; g.grid_n = w.grid_n;
    g.ld_rowpart = w.ld_rowpart;
    g.A0 = w.Ab; g.lda = w.Lp; g.a_plane0 = w.plane;
    g.B0 = m.Wtb; g.ldb = m.ldWt; g.b_plane0 = m.planeWt;
    g.M = rows; g.N = p->n_hid; g.K = m.Kv;
    g.nseg = pb_codes(ctx, v_pieces, 3, 0u, &g.seg_codes, 0);
    g.nkt = g.K / 64; g.inv_nkt = inv_of(g.nkt);
    g.kt_total = g.nseg * g.nkt; g.kt_per_split = g.kt_total; g.nsplit = 1;
    g.m_fastest = 1;
    g.bias = p->b_h;
    g.rowpart = w.rowpart;
    HIP_TRY(launch_pb(ctx, EPI_SOFTPLUS, g, st));
    FinishArgs f;
    f.v = v; f.b_v = p->b_v; f.rowpart = g.rowpart; f.F = F;
    f.rows = rows; f.n_vis = p->n_vis; f.ldv = ldv; f.ncol_tiles = g.grid_n; f.ld_rowpart = g.ld_rowpart;
    HIP_TRY(launch_free_energy_finish(f, st));
    return KURBM_OK;
}

int kurbm_score_x3(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v_batch, int v_pieces,
                   int rows, int ldv, const kurbm_cd_opts* o, float* score, float* F, void* workspace, size_t workspace_bytes,
                   kurbm_stream_t stream) {
    // rbm.py:225-233 in one call, nothing returned to the host: h ~ p(h | v) [half step, which also leaves the softplus row sums
    // of F(v): same accumulators], v' ~ p(v | h) [half step; its row-major plane feeds the next GEMM, an fp32 copy the v'.b_v
    // term], F(v') [GEMM + softplus row sums], then |F - F'| per row and its mean into *score.  Draws: chain o->chain, sites 0 (h) and 1 (v'), step o->step -- the
    // counters RBM._score has always used.
    if (!score || !aligned16(score)) return fail_msg(KURBM_ERR_ARG, "score is null or misaligned");
    if (int e = check_cd_args(ctx, 3, v_pieces, p, mirror, mirror_bytes, v_batch, rows, ldv, o, workspace, workspace_bytes, false)) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PlaneFormats pf = plane_formats(&ctx->plan, 3, v_pieces, o->mode, p->n_vis);
    const Mirror m = carve_mirror(&ctx->plan, mirror, p->n_vis, p->n_hid, 3);
    WorkspaceB w = carve_bf16(&ctx->plan, workspace, rows, p->n_vis, p->n_hid, 3, pf.v_pieces);
    const auto [act_h, act_v, noise_v] = mode_acts(pf.gauss);
    const uint32_t base = o->chain * 64u;
    // row partials of the two free energies (one row per 64- or 128-column tile), then |F - F'| per row
    const int ncol = ceil_div(p->n_hid, 128), ncol_max = ceil_div(p->n_hid, 64), ld_rp = round_up(rows, 4);
    float* rp0 = w.rowpart; float* rp1 = rp0 + (size_t)ncol_max * ld_rp; float* absdiff = rp1 + (size_t)ncol_max * ld_rp;
    if (!aligned16(p->b_v)) return fail_msg(KURBM_ERR_ARG, "b_v must be 16-byte aligned for the score");
    if (o->v_planes) w.vb = carve_vplanes(&ctx->plan, o->v_planes, rows, p->n_vis, pf.v_pieces).vb;
    else
        HIP_TRY(launch_f32_to_bf16(v_batch, rows, p->n_vis, ldv, w.vb, w.Lv, w.Kb, nullptr, 0, 0, pf.v_pieces, w.planeV, 0, nullptr, 0, st,
                                   0, pf.vbytes ? 1 : 0));
    int e;
    int ncol0 = ncol;
    RngArgs r = make_rng(o->seed, o->row0, base + 0u, o->step);
    {
        // h ~ p(h | v) AND the softplus row sums of F(v), from the same accumulators: one GEMM for rbm.py:227 and :230
        HalfOutB ho;
        ho.out = w.hb; ho.ldo = w.Lh; ho.out_bytes = pf.hbytes;
        ho.rowpart = rp0; ho.ld_rowpart = ld_rp; ho.grid_n_out = &ncol0;
        if ((e = half_step_b(ctx, LAYOUT_VH, p, m, w.vb, w.Lv, pf.v_pieces, w.planeV, rows, act_h, NOISE_BERNOULLI, &r, ho, st, pf.vbytes)))
            return e;                                                                                  // h          rbm.py:230
    }
    r = make_rng(o->seed, o->row0, base + 1u, o->step);
    {
        HalfOutB ho;
        ho.out = w.v2b; ho.ldo = w.Lv; ho.out_pieces = pf.vn_pieces; ho.out_plane = w.planeV; ho.out_bytes = pf.nbytes;
        // (a 0/1 reconstruction: the score kernel takes v'.b_v from the byte plane; real-valued v' also leaves as fp32)
        if (!pf.nbytes) { ho.out_f32 = w.tmp32; ho.ldo32 = w.ldv32; }
        if ((e = half_step_b(ctx, LAYOUT_HV, p, m, w.hb, w.Lh, 1, 0, rows, act_v, noise_v, &r, ho, st, pf.hbytes))) return e;   // v'
    }
    int ncol1 = ncol;
    {
        // F(v'): the same GEMM as a half step that draws nothing and stores nothing but its softplus row sums     rbm.py:231
        HalfOutB ho;
        ho.rowpart = rp1; ho.ld_rowpart = ld_rp; ho.grid_n_out = &ncol1;
        if ((e = half_step_b(ctx, LAYOUT_VH, p, m, w.v2b, w.Lv, pf.vn_pieces, w.planeV, rows, ACT_SIGMOID, NOISE_NONE, nullptr, ho, st, pf.nbytes))) return e;
    }
    ScoreArgs a;
    memset(&a, 0, sizeof a);
    if (pf.nbytes) { a.v1b = reinterpret_cast<const unsigned char*>(w.v2b); a.ldv1b = w.Lv; }
    a.v = v_batch; a.v1 = w.tmp32; a.b_v = p->b_v; a.rowpart = rp0; a.rowpart1 = rp1; a.F = F; a.absdiff = absdiff; a.score = score;
    a.rows = rows; a.n_vis = p->n_vis; a.ldv = ldv; a.ldv1 = w.ldv32; a.ncol_tiles = ncol0; a.ncol_tiles1 = ncol1; a.ld_rowpart = ld_rp;
    HIP_TRY(launch_score(a, st));                                                                      // mean |F - F'|  rbm.py:233
    return KURBM_OK;
}

int kurbm_x3_dump_plane(kurbm_ctx* ctx, int which, int rows, int n_vis, int n_hid, int v_pieces, int mode, const void* workspace,
                        size_t workspace_bytes, float* out, int ld_out, kurbm_stream_t stream) {
    // the planes the last complete kurbm_cd_step_x3 on (rows, v_pieces, mode) left in `workspace`, decoded to fp32 [rows][units]
    if (!ctx || !workspace || !out) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (rows <= 0 || n_vis <= 0 || n_hid <= 0 || (v_pieces != 1 && v_pieces != 3 && v_pieces != (1 | KURBM_V_BINARY)))
        return fail_msg(KURBM_ERR_ARG, "bad shape / v_pieces");
    const size_t need = carve_bf16(&ctx->plan, nullptr, rows, n_vis, n_hid, 3, v_pieces == 3 ? 3 : 1).bytes;
    if (need > workspace_bytes) return fail_msg(KURBM_ERR_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    const PlaneView v = plane_view(&ctx->plan, workspace, which, rows, n_vis, n_hid, v_pieces, mode);
    if (!v.units) return fail_msg(KURBM_ERR_ARG, "unknown plane %d", which);
    if (ld_out < v.units) return fail_msg(KURBM_ERR_ARG, "ld_out < units");
    DumpArgs a;
    memset(&a, 0, sizeof a);
    a.out = out; a.rows = rows; a.ld_out = ld_out;
    a.src = v.src; a.units = v.units; a.ld = v.ld; a.fmt = v.fmt; a.transposed = v.transposed; a.pieces = v.pieces; a.plane = v.plane;
    a.sign = v.sign;
    HIP_TRY(launch_dump_plane(a, static_cast<hipStream_t>(stream)));
    return KURBM_OK;
}

int kurbm_x3_apply_delta(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* delta,
                         float lr, int which, kurbm_stream_t stream) {
    return x3_apply_delta_any(ctx, p, mirror, mirror_bytes, delta, lr, which, stream, nullptr);
}

int kurbm_x3_apply_delta_mom(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* delta,
                             float lr, int which, kurbm_stream_t stream, const kurbm_momentum* mom) {
    if (int e = check_mom(mom, nullptr)) return e;
    return x3_apply_delta_any(ctx, p, mirror, mirror_bytes, delta, lr, which, stream, mom);
}

size_t kurbm_x3_planes_bytes(kurbm_ctx* ctx, int rows, int n_vis, int v_pieces) {
    if (v_pieces == (1 | KURBM_V_BINARY)) v_pieces = 1;
    if (!ctx || rows <= 0 || n_vis <= 0 || (v_pieces != 1 && v_pieces != 3)) return 0;
    return carve_vplanes(&ctx->plan, nullptr, rows, n_vis, v_pieces).bytes;
}

int kurbm_x3_convert_rows(kurbm_ctx* ctx, const float* v, int rows, int ldv, int n_vis, int v_pieces, void* planes,
                          size_t planes_bytes, kurbm_stream_t stream) {
    if (!ctx) return fail_msg(KURBM_ERR_ARG, "ctx is null");
    if (rows <= 0 || n_vis <= 0 || (v_pieces != 1 && v_pieces != 3 && v_pieces != (1 | KURBM_V_BINARY)))
        return fail_msg(KURBM_ERR_ARG, "bad shape / v_pieces");
    if (bad_matrix(v, ldv, n_vis)) return fail_msg(KURBM_ERR_ARG, "v: null, misaligned, ld %% 4 != 0 or ld < n_vis");
    // 0/1 data: the transposed plane (operand of the positive statistics only) as fp8 and the row-major one as bytes, as the steps
    // will read them (neither depends on the mode)
    const PlaneFormats pf = plane_formats(&ctx->plan, 3, v_pieces, KURBM_MODE_VISIBLE_BERNOULLI, n_vis);
    const VPlanes vp = carve_vplanes(&ctx->plan, planes, rows, n_vis, pf.v_pieces);
    if (int e = check_buffer("planes", planes, vp.bytes, planes_bytes)) return e;
    const int Kb = round_up(rows, 128), Lv = ld_pad(&ctx->plan, round_up(n_vis, 128)), Lb = ld_pad(&ctx->plan, Kb);
    HIP_TRY(launch_f32_to_bf16(v, rows, n_vis, ldv, vp.vb, Lv, Kb, vp.vbT, Lb, n_vis, pf.v_pieces, (size_t)Kb * Lv, (size_t)n_vis * Lb,
                               vp.part_v, round_up(n_vis, 4), static_cast<hipStream_t>(stream), pf.f8pos ? 1 : 0, pf.vbytes ? 1 : 0));
    return KURBM_OK;
}

}  // extern "C"
