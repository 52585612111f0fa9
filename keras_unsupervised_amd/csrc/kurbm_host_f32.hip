// kurbm_host_f32.hip -- the fp32 path of the C ABI (include/kurbm.h): half steps, the CD step and its one-launch form for small
// RBMs, label units, class logits, discriminative / hybrid training, free energy, AIS and the statistics GEMM on its own.
// Launch sequences only: planning and layouts are in kurbm_plan.h, the checks in kurbm_host.h, all arithmetic in the kernels.
#include "kurbm_host.h"

using namespace kurbm;

// ---- the half step ---------------------------------------------------------------------
static int half_step(kurbm_ctx* ctx, int layout, const kurbm_params* p, const float* in, int rows, int ld_in,
                     int act, int noise, const RngArgs* rng, float* out_sample, float* out_prob, float* out_u,
                     int ldo, const float* ref, int ldref, float* colpart, int ld_colpart, int* grid_m_out,
                     hipStream_t st, int* cfg_out = nullptr) {
    const int K = (layout == LAYOUT_VH) ? p->n_vis : p->n_hid;
    const int N = (layout == LAYOUT_VH) ? p->n_hid : p->n_vis;
    if (int e = check_batch(in, rows, ld_in, K, "input")) return e;
    if (act < ACT_SIGMOID || act > ACT_LINEAR) return fail_msg(KURBM_ERR_ARG, "unknown activation %d", act);
    if (noise < NOISE_NONE || noise > NOISE_GAUSSIAN) return fail_msg(KURBM_ERR_ARG, "unknown noise %d", noise);
    if (!out_sample && !out_prob) return fail_msg(KURBM_ERR_ARG, "both outputs are null");
    if (noise != NOISE_NONE && !rng) return fail_msg(KURBM_ERR_ARG, "rng is null");
    if (noise != NOISE_NONE && (rng->row0 & 3)) return fail_msg(KURBM_ERR_ARG, "rng.row0 must be a multiple of 4");
    if (noise == NOISE_NONE && out_sample && !out_prob) { out_prob = out_sample; out_sample = nullptr; }
    if ((out_sample && bad_matrix(out_sample, ldo, N)) || (out_prob && bad_matrix(out_prob, ldo, N)))
        return fail_msg(KURBM_ERR_ARG, "output: misaligned, ld %% 4 != 0 or ld < columns");

    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A0 = in; g.lda = ld_in;
    g.B0 = p->W; g.ldb = p->ldw;
    g.M = rows; g.N = N; g.K = K;
    g.nseg = 1;
    g.nkt = K / 32;
    g.kt_total = g.nkt; g.kt_per_split = g.nkt; g.nsplit = 1;
    const int cfg = pick_cfg(ctx->plan.ncu, rows, N, &g.grid_m, &g.grid_n, force_cfg(&ctx->plan, layout));
    g.bias = (layout == LAYOUT_VH) ? p->b_h : p->b_v;
    g.out_sample = out_sample; g.out_prob = out_prob; g.out_u = out_u; g.ldo = ldo;
    g.ref = ref; g.ldref = ldref; g.colpart = colpart; g.ld_colpart = ld_colpart;
    g.act = act; g.noise = noise;
    if (rng) g.rng = *rng;
    g.m_fastest = (g.grid_m < g.grid_n) ? 1 : 0;
    if (grid_m_out) *grid_m_out = g.grid_m;
    if (cfg_out) *cfg_out = cfg;
    HIP_TRY(launch_gemm(layout, cfg, EPI_HALFSTEP, g, st));
    return KURBM_OK;
}
// ... with nothing but its value plane: samples (noise) or probabilities / pre-activations (NOISE_NONE)
static int half_step_plain(kurbm_ctx* ctx, int layout, const kurbm_params* p, const float* in, int rows, int ld_in, int act, int noise,
                           const RngArgs* rng, float* out, int ldo, hipStream_t st) {
    return half_step(ctx, layout, p, in, rows, ld_in, act, noise, rng, noise == NOISE_NONE ? nullptr : out, noise == NOISE_NONE ? out : nullptr,
                     nullptr, ldo, nullptr, 0, nullptr, 0, nullptr, st);
}

// ---- the statistics GEMM and the reduction of its slabs ------------------------------------
// A1 / B1 null: one segment (plan_outer_one)
static int outer_slabs(kurbm_ctx* ctx, const float* A0, const float* B0, const float* A1, const float* B1, int rows, int m, int n_hid,
                       int lda, int ldb, float* slab, size_t slab_stride, const OuterPlan& pl, hipStream_t st) {
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A0 = A0; g.A1 = A1; g.lda = lda;
    g.B0 = B0; g.B1 = B1; g.ldb = ldb;
    g.M = m; g.N = n_hid; g.K = rows;
    g.nseg = A1 ? 2 : 1;
    g.nkt = pl.nkt; g.kt_total = pl.kt_total; g.kt_per_split = pl.kt_per_split; g.nsplit = pl.nsplit;
    g.grid_m = pl.gm; g.grid_n = pl.gn;
    g.slab = slab; g.slab_stride = slab_stride; g.ld_slab = pl.ld_slab;
    g.tile_major = knob(ctx, KN_TILE_MAJOR);
    HIP_TRY(launch_gemm(LAYOUT_OUTER, pl.cfg, EPI_SLAB, g, st));
    return KURBM_OK;
}
// The slab half of launch_reduce_apply's arguments: the slabs of `pl` summed into m x n_hid (need_w = false: no weight work).  The
// caller adds where the sums go (W / delta_w) and the bias partials; without them the bias blocks do nothing.
static ReduceArgs stats_reduce_args(const kurbm_ctx* ctx, const OuterPlan& pl, float* slab, size_t slab_stride, int m, int n_hid, int ldw,
                                    bool need_w = true) {
    ReduceArgs a;
    memset(&a, 0, sizeof a);
    a.slab = slab; a.slab_stride = slab_stride; a.nslab = pl.nsplit; a.ld_slab = pl.ld_slab;
    a.n_vis = m; a.n_hid = n_hid; a.ldw = ldw;
    a.nblk_w = need_w ? (int)(((long long)m * (pl.ld_slab / 4) + 255) / 256) : 0;
    if (need_w && knob(ctx, KN_TILE_MAJOR)) {
        tile_shape(pl.cfg, &a.tile_bm, &a.tile_bn);
        a.grid_m = pl.gm; a.grid_n = pl.gn; a.parts = 4; a.m_fastest = 0;
        a.nblk_w = pl.gm * pl.gn * a.parts;
    }
    return a;
}

// ---- softmax label units (include/kurbm.h: kurbm_label_sample) --------------------------
// The label site behind an h -> v half step (arguments checked by the caller): the block of v is redrawn; with `part` the label
// columns of that half step's visible-bias partials (row tiles of tile_h rows) are rewritten from ref - v.
static int label_site(const kurbm_params* p, int n_labels, const float* h, int rows, int ldh, const RngArgs& rng, float* v, int ldv,
                      float* prob, int ldp, float* out_u, const float* ref, int ldref, float* part, int ld_part, int tile_h,
                      hipStream_t st) {
    LabelArgs a;
    memset(&a, 0, sizeof a);
    a.h = h; a.ldh = ldh; a.W = p->W; a.ldw = p->ldw; a.b_v = p->b_v;
    a.v = v; a.ldv = ldv; a.prob = prob; a.ldp = ldp; a.out_u = out_u;
    a.ref = ref; a.ldref = ldref; a.part = part; a.ld_part = ld_part;
    a.rows = rows; a.n_pix = p->n_vis - n_labels; a.C = n_labels; a.n_hid = p->n_hid; a.tile_h = tile_h;
    a.rng = rng;
    HIP_TRY(launch_label_sample(a, st));
    return KURBM_OK;
}

// ---- the CD step -----------------------------------------------------------------------
// (mom: null = the reference's bare rule on the ordinary kernels; else kurbm_cd_step_mom.  n_labels: 0 = no label block, exactly
//  the launches of kurbm_cd_step; else kurbm_cd_step_labels: the label site runs behind every h -> v half step)
static int cd_step_f32(kurbm_ctx* ctx, const kurbm_params* p, const float* v_batch, int rows, int ldv,
                       const kurbm_cd_opts* o, int which, void* workspace, size_t workspace_bytes, kurbm_stream_t stream,
                       const kurbm_momentum* mom, int n_labels = 0) {
    if (!ctx || !o) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_params(p)) return e;
    if (n_labels) {
        if (int e = check_labels(p, n_labels)) return e;
        if (o->mode != KURBM_MODE_VISIBLE_BERNOULLI) return fail_msg(KURBM_ERR_ARG, "label units need Bernoulli visibles (mode %d)", o->mode);
    }
    if (int e = check_batch(v_batch, rows, ldv, p->n_vis)) return e;
    if (int e = check_opts(o)) return e;
    if (o->v_chain && !aligned16(o->v_chain)) return fail_msg(KURBM_ERR_ARG, "v_chain is misaligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Workspace w = carve_f32(&ctx->plan, workspace, rows, p->n_vis, p->n_hid, ldv);
    if (int e = check_workspace(workspace, w.bytes, workspace_bytes,
                                ldv > w.ldv ? " (ldv > round_up(n_vis, 4): v_neg is kept at the batch's leading dimension, see kurbm_workspace_bytes)" : ""))
        return e;

    const auto [act_h, act_v, noise_v] = mode_acts(o->mode == KURBM_MODE_VISIBLE_GAUSSIAN);
    const uint32_t base = o->chain * 64u;
    const bool need_w = (which & 1) || o->delta_out;
    int e;

    // h_pos ~ p(h | v_pos)                                        rbm.py:120 (self.transform)
    RngArgs r = make_rng(o->seed, o->row0, base + 0u, o->step);
    if ((e = half_step_plain(ctx, LAYOUT_VH, p, v_batch, rows, ldv, act_h, NOISE_BERNOULLI, &r, w.h_pos, w.ldh, st))) return e;
    const float* h_cur = w.h_pos;
    if (o->v_chain) {  // persistent chain: the negative phase starts from the stored fantasy
        r = make_rng(o->seed, o->row0, base + 32u, o->step);
        if ((e = half_step_plain(ctx, LAYOUT_VH, p, o->v_chain, rows, ldv, act_h, NOISE_BERNOULLI, &r, w.h_tmp, w.ldh, st))) return e;
        h_cur = w.h_tmp;
    }
    // the final v sample is written straight into the persistent chain when there is one
    float* v_last = o->v_chain ? o->v_chain : w.v_neg;
    int gm_v = 0, gm_h = 0;
    for (int t = 1; t <= o->k; ++t) {
        const bool last = (t == o->k);
        // v_t ~ p(v | h_{t-1})                                    rbm.py:121-123 / :143-144
        r = make_rng(o->seed, o->row0, base + 2u * t - 1u, o->step);
        float* v_out = last ? v_last : w.v_neg;
        int cfg_v = 0;
        if ((e = half_step(ctx, LAYOUT_HV, p, h_cur, rows, w.ldh, act_v, noise_v, &r, v_out, nullptr, nullptr, ldv,
                           last ? v_batch : nullptr, ldv, w.part_v, w.ld_part_v, last ? &gm_v : nullptr, st, &cfg_v)))
            return e;
        if (n_labels) {
            // the label block of v_t is one softmax draw, not C Bernoulli ones: same site, one uniform per row
            int bm, bn;
            tile_shape(cfg_v, &bm, &bn);
            if ((e = label_site(p, n_labels, h_cur, rows, w.ldh, r, v_out, ldv, nullptr, 0, nullptr, last ? v_batch : nullptr, ldv,
                                last ? w.part_v : nullptr, w.ld_part_v, bm, st)))
                return e;
        }
        if (!last) {
            r = make_rng(o->seed, o->row0, base + 2u * t, o->step);
            if ((e = half_step_plain(ctx, LAYOUT_VH, p, v_out, rows, ldv, act_h, NOISE_BERNOULLI, &r, w.h_tmp, w.ldh, st))) return e;
            h_cur = w.h_tmp;
        }
    }
    // h_neg = sigmoid(v_neg.W + b_h): probabilities, sigmoid in both modes   rbm.py:124 / :145
    if ((e = half_step(ctx, LAYOUT_VH, p, v_last, rows, ldv, ACT_SIGMOID, NOISE_NONE, nullptr, nullptr, w.h_neg, nullptr,
                       w.ldh, w.h_pos, w.ldh, w.part_h, w.ld_part_h, &gm_h, st)))
        return e;

    // dW = v_pos^T.h_pos - v_neg^T.h_neg  (rbm.py:125-126) as split-K slabs
    const OuterPlan pl = plan_outer(&ctx->plan, rows, p->n_vis, p->n_hid);
    if (need_w)
        if ((e = outer_slabs(ctx, v_batch, w.h_pos, v_last, w.h_neg, rows, p->n_vis, p->n_hid, ldv, w.ldh, w.slab,
                             w.slab_stride, pl, st)))
            return e;

    // reduce slabs / bias partials, apply lr * sums (rbm.py:127-134) and/or emit the packed delta
    ReduceArgs a = stats_reduce_args(ctx, pl, w.slab, w.slab_stride, p->n_vis, p->n_hid, p->ldw, need_w);
    reduce_targets(a, p, o, which);
    a.part_h = w.part_h; a.nrow_tiles_h = gm_h; a.ld_part_h = w.ld_part_h;
    a.part_v = w.part_v; a.nrow_tiles_v = gm_v; a.ld_part_v = w.ld_part_v;
    HIP_TRY(launch_reduce_apply(a, st, make_mom(p, mom).ptr()));
    return KURBM_OK;
}

static int cd_epoch_f32(kurbm_ctx* ctx, const kurbm_params* p, const float* V, int n_rows, int ldv, int batch_size,
                        const kurbm_cd_opts* opts, void* workspace, size_t workspace_bytes, kurbm_stream_t stream,
                        const kurbm_momentum* mom, int n_labels = 0) {
    if (int e = check_epoch(ctx, opts, n_rows, batch_size)) return e;
    if (opts->delta_out || !opts->apply) return fail_msg(KURBM_ERR_ARG, "kurbm_cd_epoch applies in place: apply = 1, delta_out = null");
    kurbm_cd_opts o = *opts;
    return for_each_batch(n_rows, batch_size, [&](int lo, int rows, int) {
        const int e = cd_step_f32(ctx, p, V + (size_t)lo * ldv, rows, ldv, &o, 7, workspace, workspace_bytes, stream, mom, n_labels);
        ++o.step;
        return e;
    });
}

// ---- the one-launch step and score of a small RBM (kurbm_small.hip) ----------------------------
// What both launches share of SmallArgs, and *nblk: enough workgroups for the widest phase (one 16 x 16 tile of a half step per
// workgroup; `extra`: another phase's need), never more than the CUs -- the grid must be resident, one workgroup per CU
static SmallArgs small_args(const kurbm_ctx* ctx, const kurbm_params* p, const float* v_batch, int rows, int ldv, const kurbm_cd_opts* o,
                            const Workspace& w, int extra, int* nblk) {
    SmallArgs a;
    memset(&a, 0, sizeof a);
    a.W = p->W; a.b_h = p->b_h; a.b_v = p->b_v; a.n_vis = p->n_vis; a.n_hid = p->n_hid; a.ldw = p->ldw;
    a.v = v_batch; a.rows = rows; a.ldv = ldv;
    a.h_pos = w.h_pos; a.h_neg = w.h_neg; a.v_neg = w.v_neg; a.ldh = w.ldh; a.ldn = w.ldv;
    a.ldt = round_up(rows, 16);
    a.h_posT = w.small_t;
    a.bar = ctx->status + 64; a.status = ctx->status;
    a.timeout_ticks = 200000000ull;          // 2 s of the 100 MHz clock: only a grid that is not resident ever gets there
    const uint32_t base = o->chain * 64u;
    a.rng_h = make_rng(o->seed, o->row0, base + 0u, o->step);
    a.rng_v = make_rng(o->seed, o->row0, base + 1u, o->step);
    a.gauss = (o->mode == KURBM_MODE_VISIBLE_GAUSSIAN) ? 1 : 0;
    const int ncu = ctx->plan.ncu;
    const int tm = ceil_div(rows, 16), tv = ceil_div(p->n_vis, 16), th = ceil_div(p->n_hid, 16);
    *nblk = tm * th > tm * tv ? tm * th : tm * tv;
    if (extra > *nblk) *nblk = extra;
    if (*nblk > ncu) *nblk = ncu;
    // the XCD-local schedule: every XCD's workgroups own the row tiles tm = its number (mod 8), so the whole grid is launched
    a.local = (knob(ctx, KN_SMALL_LOCAL) != 0 && ctx->xcc_round_robin && ncu <= 256) ? 1 : 0;   // (a group's barrier: 32 words)
    a.xcc_map = ctx->xcc_map;
    if (a.local) *nblk = ncu;
    return a;
}

extern "C" {

int kurbm_half_step_vh(kurbm_ctx* ctx, const kurbm_params* p, const float* v, int rows, int ldv, int act, int noise,
                       const kurbm_rng* rng, float* out_sample, float* out_prob, int ldh, kurbm_stream_t stream) {
    return kurbm_half_step_vh_dbg(ctx, p, v, rows, ldv, act, noise, rng, out_sample, out_prob, nullptr, ldh, stream);
}

int kurbm_half_step_hv(kurbm_ctx* ctx, const kurbm_params* p, const float* h, int rows, int ldh, int act, int noise,
                       const kurbm_rng* rng, float* out_sample, float* out_prob, int ldv, kurbm_stream_t stream) {
    return kurbm_half_step_hv_dbg(ctx, p, h, rows, ldh, act, noise, rng, out_sample, out_prob, nullptr, ldv, stream);
}

static int half_step_dbg(kurbm_ctx* ctx, int layout, const kurbm_params* p, const float* in, int rows, int ld_in, int act, int noise,
                         const kurbm_rng* rng, float* out_sample, float* out_prob, float* out_u, int ldo, kurbm_stream_t stream) {
    if (!ctx) return fail_msg(KURBM_ERR_ARG, "ctx is null");
    if (int e = check_params(p)) return e;
    RngArgs r;
    if (rng) r = make_rng(rng);
    return half_step(ctx, layout, p, in, rows, ld_in, act, noise, rng ? &r : nullptr, out_sample, out_prob, out_u, ldo,
                     nullptr, 0, nullptr, 0, nullptr, static_cast<hipStream_t>(stream));
}

int kurbm_half_step_vh_dbg(kurbm_ctx* ctx, const kurbm_params* p, const float* v, int rows, int ldv, int act,
                           int noise, const kurbm_rng* rng, float* out_sample, float* out_prob, float* out_u, int ldh,
                           kurbm_stream_t stream) {
    return half_step_dbg(ctx, LAYOUT_VH, p, v, rows, ldv, act, noise, rng, out_sample, out_prob, out_u, ldh, stream);
}

int kurbm_half_step_hv_dbg(kurbm_ctx* ctx, const kurbm_params* p, const float* h, int rows, int ldh, int act,
                           int noise, const kurbm_rng* rng, float* out_sample, float* out_prob, float* out_u, int ldv,
                           kurbm_stream_t stream) {
    return half_step_dbg(ctx, LAYOUT_HV, p, h, rows, ldh, act, noise, rng, out_sample, out_prob, out_u, ldv, stream);
}

size_t kurbm_workspace_bytes(kurbm_ctx* ctx, int rows, int n_vis, int n_hid, int k) {
    (void)k;
    if (!ctx || rows <= 0 || n_vis <= 0 || n_hid <= 0) return 0;
    return carve_f32(&ctx->plan, nullptr, rows, n_vis, n_hid).bytes;
}

int kurbm_cd_step(kurbm_ctx* ctx, const kurbm_params* p, const float* v_batch, int rows, int ldv,
                  const kurbm_cd_opts* o, int which, void* workspace, size_t workspace_bytes, kurbm_stream_t stream) {
    return cd_step_f32(ctx, p, v_batch, rows, ldv, o, which, workspace, workspace_bytes, stream, nullptr);
}

int kurbm_cd_step_mom(kurbm_ctx* ctx, const kurbm_params* p, const float* v_batch, int rows, int ldv,
                      const kurbm_cd_opts* o, int which, void* workspace, size_t workspace_bytes, kurbm_stream_t stream,
                      const kurbm_momentum* mom) {
    if (!o) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_mom(mom, o)) return e;
    return cd_step_f32(ctx, p, v_batch, rows, ldv, o, which, workspace, workspace_bytes, stream, mom);
}

// One CD-1 update of a small RBM in ONE launch (kurbm_small.hip).  Workspace as kurbm_cd_step (kurbm_workspace_bytes).
int kurbm_cd_step_small(kurbm_ctx* ctx, const kurbm_params* p, const float* v_batch, int rows, int ldv, const kurbm_cd_opts* o,
                        int which, void* workspace, size_t workspace_bytes, kurbm_stream_t stream) {
    if (!ctx || !o) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_params(p)) return e;
    if (int e = check_batch(v_batch, rows, ldv, p->n_vis)) return e;
    if (o->k != 1 || o->v_chain || !o->apply || o->delta_out)
        return fail_msg(KURBM_ERR_UNSUPPORTED, "kurbm_cd_step_small runs CD-1 from the data, applied in place (k = 1, no v_chain, apply = 1, no delta_out)");
    if (int e = check_opts(o, false)) return e;
    const Workspace w = carve_f32(&ctx->plan, workspace, rows, p->n_vis, p->n_hid);
    if (int e = check_workspace(workspace, w.bytes, workspace_bytes)) return e;
    if (rows > SMALL_ROWS_MAX) return fail_msg(KURBM_ERR_UNSUPPORTED, "kurbm_cd_step_small: at most %d rows per batch", SMALL_ROWS_MAX);
    // (the statistics phase: one tile of W per wave, eight waves per workgroup: kurbm_small.hip SMALL_WAVES)
    const int tv = ceil_div(p->n_vis, 16), th = ceil_div(p->n_hid, 16);
    int nblk;
    SmallArgs a = small_args(ctx, p, v_batch, rows, ldv, o, w, ceil_div(tv * th + tv + th, 8), &nblk);
    a.h_negT = a.h_posT + (size_t)p->n_hid * a.ldt; a.v_negT = a.h_negT + (size_t)p->n_hid * a.ldt;
    a.which = which; a.lr = o->lr;
    if (nblk > 1024) nblk = 1024;
    HIP_TRY(launch_cd1_small(a, nblk, static_cast<hipStream_t>(stream)));
    return KURBM_OK;
}

// The per-step score of fit(verbose = 1) for a small RBM in ONE launch (kurbm_small.hip: k_score_small).
int kurbm_score_small(kurbm_ctx* ctx, const kurbm_params* p, const float* v_batch, int rows, int ldv, const kurbm_cd_opts* o,
                      float* score, float* F, void* workspace, size_t workspace_bytes, kurbm_stream_t stream) {
    if (!ctx || !o || !score) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(score) & 7) return fail_msg(KURBM_ERR_ARG, "score must be 8-byte aligned (two floats are written)");
    if (int e = check_params(p)) return e;
    if (rows <= 0 || rows > SMALL_ROWS_MAX) return fail_msg(KURBM_ERR_ARG, "rows must be in [1, %d]", SMALL_ROWS_MAX);
    if (int e = check_batch(v_batch, rows, ldv, p->n_vis)) return e;
    if (int e = check_opts(o, false)) return e;
    const Workspace w = carve_f32(&ctx->plan, workspace, rows, p->n_vis, p->n_hid);
    if (int e = check_workspace(workspace, w.bytes, workspace_bytes)) return e;
    int nblk;
    SmallArgs a = small_args(ctx, p, v_batch, rows, ldv, o, w, 0, &nblk);     // (the row partials live in the transposed planes' space)
    a.score = score; a.F = F;
    HIP_TRY(launch_score_small(a, nblk, static_cast<hipStream_t>(stream)));
    return KURBM_OK;
}

// An epoch of fit(verbose = 1) for a small RBM in one call: every batch's update followed by its score (rbm.py:211-234), two
// launches per step, nothing read back -- scores[2 * step] receives the score and scores[2 * step + 1] a 1.0f when it has landed
// (device memory, or pinned host memory that the caller polls while the device runs on).  Returns the number of steps.
int kurbm_cd_epoch_small_scored(kurbm_ctx* ctx, const kurbm_params* p, const float* V, int n_rows, int ldv, int batch_size,
                                const kurbm_cd_opts* opts, int score_chain, float* scores, void* workspace, size_t workspace_bytes,
                                kurbm_stream_t stream) {
    if (!scores) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_epoch(ctx, opts, n_rows, batch_size)) return e;
    kurbm_cd_opts o = *opts, so = *opts;
    so.chain = score_chain;
    return for_each_batch(n_rows, batch_size, [&](int lo, int rows, int step) {
        if (int e = kurbm_cd_step_small(ctx, p, V + (size_t)lo * ldv, rows, ldv, &o, 7, workspace, workspace_bytes, stream)) return e;
        if (int e = kurbm_score_small(ctx, p, V + (size_t)lo * ldv, rows, ldv, &so, scores + 2 * (size_t)step, nullptr, workspace,
                                      workspace_bytes, stream)) return e;
        ++o.step; ++so.step;
        return (int)KURBM_OK;
    });
}

int kurbm_cd_epoch_small(kurbm_ctx* ctx, const kurbm_params* p, const float* V, int n_rows, int ldv, int batch_size,
                         const kurbm_cd_opts* opts, void* workspace, size_t workspace_bytes, kurbm_stream_t stream) {
    if (int e = check_epoch(ctx, opts, n_rows, batch_size)) return e;
    kurbm_cd_opts o = *opts;
    return for_each_batch(n_rows, batch_size, [&](int lo, int rows, int) {
        const int e = kurbm_cd_step_small(ctx, p, V + (size_t)lo * ldv, rows, ldv, &o, 7, workspace, workspace_bytes, stream);
        ++o.step;
        return e;
    });
}

int kurbm_cd_epoch(kurbm_ctx* ctx, const kurbm_params* p, const float* V, int n_rows, int ldv, int batch_size,
                   const kurbm_cd_opts* opts, void* workspace, size_t workspace_bytes, kurbm_stream_t stream) {
    return cd_epoch_f32(ctx, p, V, n_rows, ldv, batch_size, opts, workspace, workspace_bytes, stream, nullptr);
}

int kurbm_cd_epoch_mom(kurbm_ctx* ctx, const kurbm_params* p, const float* V, int n_rows, int ldv, int batch_size,
                       const kurbm_cd_opts* opts, void* workspace, size_t workspace_bytes, kurbm_stream_t stream,
                       const kurbm_momentum* mom) {
    if (!opts) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_mom(mom, opts)) return e;
    return cd_epoch_f32(ctx, p, V, n_rows, ldv, batch_size, opts, workspace, workspace_bytes, stream, mom);
}

// ---- softmax label units: the entry points -------------------------------------------------
int kurbm_label_sample(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* h, int rows, int ldh, const kurbm_rng* rng,
                       float* v, int ldv, float* prob, int ldp, float* out_u, kurbm_stream_t stream) {
    if (!ctx || !rng) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_params(p)) return e;
    if (int e = check_labels(p, n_labels)) return e;
    if (int e = check_batch(h, rows, ldh, p->n_hid, "h")) return e;
    if (int e = check_batch(v, rows, ldv, p->n_vis, "v")) return e;
    if (prob && bad_matrix(prob, ldp, n_labels)) return fail_msg(KURBM_ERR_ARG, "prob: misaligned, ld %% 4 != 0 or ld < n_labels");
    if (rng->row0 & 3) return fail_msg(KURBM_ERR_ARG, "rng.row0 must be a multiple of 4");
    return label_site(p, n_labels, h, rows, ldh, make_rng(rng), v, ldv, prob, ldp, out_u, nullptr, 0, nullptr, 0, 128,
                      static_cast<hipStream_t>(stream));
}

// (the label entry points: the parameter block, the label count and a given momentum block, before the step's own checks)
static int check_label_entry(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const kurbm_cd_opts* o, const kurbm_momentum* mom) {
    if (!ctx || !o) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_params(p)) return e;
    if (int e = check_labels(p, n_labels)) return e;
    return mom ? check_mom(mom, o) : (int)KURBM_OK;
}

int kurbm_cd_step_labels(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* v_batch, int rows, int ldv,
                         const kurbm_cd_opts* o, int which, void* workspace, size_t workspace_bytes, kurbm_stream_t stream,
                         const kurbm_momentum* mom) {
    if (int e = check_label_entry(ctx, p, n_labels, o, mom)) return e;
    return cd_step_f32(ctx, p, v_batch, rows, ldv, o, which, workspace, workspace_bytes, stream, mom, n_labels);
}

int kurbm_cd_epoch_labels(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* V, int n_rows, int ldv, int batch_size,
                          const kurbm_cd_opts* opts, void* workspace, size_t workspace_bytes, kurbm_stream_t stream,
                          const kurbm_momentum* mom) {
    if (int e = check_label_entry(ctx, p, n_labels, opts, mom)) return e;
    return cd_epoch_f32(ctx, p, V, n_rows, ldv, batch_size, opts, workspace, workspace_bytes, stream, mom, n_labels);
}

size_t kurbm_class_workspace_bytes(kurbm_ctx* ctx, int rows, int n_vis, int n_hid) {
    if (!ctx || rows <= 0 || n_vis <= 0 || n_hid <= 0) return 0;
    return carve_class(nullptr, rows, n_hid).bytes;
}

}  // extern "C"

// a = v.W[:n_pix] + b_h: the linear half step on a parameter block that ends at the pixel rows (they are W's top rows: nothing is
// copied), then k_class_logits on it
static int class_logit_launches(kurbm_ctx* ctx, const kurbm_params* p, int C, const float* v, int rows, int ldv, float* a_plane, int lda,
                                float* logits, float* prob, int ldl, hipStream_t st) {
    kurbm_params pp = *p;
    pp.n_vis = p->n_vis - C;
    if (int e = half_step_plain(ctx, LAYOUT_VH, &pp, v, rows, ldv, ACT_LINEAR, NOISE_NONE, nullptr, a_plane, lda, st)) return e;
    ClassLogitArgs c;
    memset(&c, 0, sizeof c);
    c.a = a_plane; c.lda = lda; c.W = p->W; c.ldw = p->ldw; c.b_v = p->b_v;
    c.logits = logits; c.prob = prob; c.ldl = ldl;
    c.rows = rows; c.n_pix = pp.n_vis; c.C = C; c.n_hid = p->n_hid;
    HIP_TRY(launch_class_logits(c, st));
    return KURBM_OK;
}

extern "C" int kurbm_class_logits(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* v, int rows, int ldv, float* logits,
                                  int ldl, float* prob, void* workspace, size_t workspace_bytes, kurbm_stream_t stream) {
    if (!ctx) return fail_msg(KURBM_ERR_ARG, "ctx is null");
    if (int e = check_params(p)) return e;
    if (int e = check_labels(p, n_labels)) return e;
    if (int e = check_batch(v, rows, ldv, p->n_vis - n_labels, "v")) return e;
    if (bad_matrix(logits, ldl, n_labels)) return fail_msg(KURBM_ERR_ARG, "logits: null, misaligned, ld %% 4 != 0 or ld < n_labels");
    if (prob && !aligned16(prob)) return fail_msg(KURBM_ERR_ARG, "prob is misaligned");
    const ClassWorkspace w = carve_class(workspace, rows, p->n_hid);
    if (int e = check_workspace(workspace, w.bytes, workspace_bytes)) return e;
    return class_logit_launches(ctx, p, n_labels, v, rows, ldv, w.a, w.lda, logits, prob, ldl, static_cast<hipStream_t>(stream));
}

namespace kurbm {
int apply_delta_f32(kurbm_ctx* ctx, const kurbm_params* p, const float* delta, float lr, int which,
                    kurbm_stream_t stream, const kurbm_momentum* mom) {
    if (!ctx || !delta) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_params(p)) return e;
    ApplyArgs a;
    a.delta = delta;
    a.W = (which & 1) ? p->W : nullptr;
    a.b_h = (which & 2) ? p->b_h : nullptr;
    a.b_v = (which & 4) ? p->b_v : nullptr;
    a.n_vis = p->n_vis; a.n_hid = p->n_hid; a.ldw = p->ldw; a.lr = lr;
    HIP_TRY(launch_apply_delta(a, static_cast<hipStream_t>(stream), make_mom(p, mom).ptr()));
    return KURBM_OK;
}
}  // namespace kurbm

// ---- discriminative and hybrid training of a label RBM (include/kurbm.h: kurbm_disc_step) -----------------------------
// what every entry point of the family refuses, before anything is enqueued
static int check_disc(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* v_batch, int rows, int ldv, const void* ws) {
    if (!ctx) return fail_msg(KURBM_ERR_ARG, "ctx is null");
    if (int e = check_params(p)) return e;
    if (int e = check_labels(p, n_labels)) return e;
    if (int e = check_batch(v_batch, rows, ldv, p->n_vis)) return e;
    return check_workspace(ws, 0, 0);
}

// The launches of one gradient (arguments checked by the caller): the linear half step on the pixel rows of W, k_class_logits,
// k_class_grad, the statistics GEMM v_pix^T.g (one segment) with the reduction of its slabs into the pixel rows of delta's dW, then
// k_class_reduce for the rest of the packed delta (+ gen_weight * gen everywhere, when gen is given).  S_y / H_bar (nullable,
// leading dimension ldh): the caller's planes.
static int class_grad_launches(kurbm_ctx* ctx, const kurbm_params* p, int C, const float* v_batch, int rows, int ldv,
                               const DiscWorkspace& w, float* S_y, float* H_bar, int ldh, float* nll, float* delta, const float* gen,
                               float gen_weight, float* nll_mean, hipStream_t st, int stage = 0) {
    const int n_pix = p->n_vis - C, n_hid = p->n_hid;
    // (stage: the measurement knob KURBM_DISC_STAGE -- one group of the launches, on what a complete call left in the workspace)
    const bool s1 = stage == 0 || stage == 1, s2 = stage == 0 || stage == 2, s3 = stage == 0 || stage == 3;
    if (s1)
        if (int e = class_logit_launches(ctx, p, C, v_batch, rows, ldv, w.a, w.ldh, w.logits, w.prob, w.ldl, st)) return e;
    ClassGradArgs g;
    memset(&g, 0, sizeof g);
    g.a = w.a; g.lda = w.ldh; g.W = p->W; g.ldw = p->ldw;
    g.logits = w.logits; g.prob = w.prob; g.ldl = w.ldl;
    g.v = v_batch; g.ldv = ldv;
    g.g = w.g; g.ldg = w.ldh;
    g.S_y = S_y; g.H_bar = H_bar; g.ldh = ldh;
    g.nll = nll ? nll : w.nll;
    g.part = w.part; g.ld_part = w.ld_part; g.part_d = w.part_d;
    g.rows = rows; g.n_pix = n_pix; g.C = C; g.n_hid = n_hid;
    if (s2) HIP_TRY(launch_class_grad(g, st));
    if (!s3) return KURBM_OK;
    // dW[:n_pix] = v_pix^T.S_y - v_pix^T.H_bar = v_pix^T.g: the statistics GEMM with one segment, M = n_pix
    const OuterPlan pl = plan_outer_one(&ctx->plan, rows, n_pix, n_hid);
    if (int e = outer_slabs(ctx, v_batch, w.g, nullptr, nullptr, rows, n_pix, n_hid, ldv, w.ldh, w.slab, w.slab_stride, pl, st)) return e;
    ReduceArgs a = stats_reduce_args(ctx, pl, w.slab, w.slab_stride, n_pix, n_hid, 0);
    a.delta_w = delta;
    HIP_TRY(launch_reduce_apply(a, st));     // (no bias work: null partial pointers)
    ClassReduceArgs r;
    memset(&r, 0, sizeof r);
    r.part = w.part; r.ld_part = w.ld_part; r.part_d = w.part_d; r.ntiles = w.ntiles;
    r.nll = g.nll; r.nll_mean = nll_mean; r.rows = rows;
    r.delta = delta; r.gen = gen; r.gen_weight = gen_weight;
    r.n_pix = n_pix; r.C = C; r.n_hid = n_hid;
    HIP_TRY(launch_class_reduce(r, st));
    return KURBM_OK;
}

static int disc_step_f32(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* v_batch, int rows, int ldv,
                         const kurbm_cd_opts* o, float gen_weight, float* nll_mean, void* ws, size_t ws_bytes, kurbm_stream_t stream,
                         const kurbm_momentum* mom) {
    if (!o) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_disc(ctx, p, n_labels, v_batch, rows, ldv, ws)) return e;
    if (!(gen_weight >= 0.f && gen_weight <= 3.4028235e38f)) return fail_msg(KURBM_ERR_ARG, "gen_weight must be finite and >= 0, got %g", (double)gen_weight);
    if (o->mode != KURBM_MODE_VISIBLE_BERNOULLI) return fail_msg(KURBM_ERR_ARG, "label units need Bernoulli visibles (mode %d)", o->mode);
    if (nll_mean && (reinterpret_cast<uintptr_t>(nll_mean) & 3u)) return fail_msg(KURBM_ERR_ARG, "nll_mean is misaligned");
    if (mom)
        if (int e = check_mom(mom, nullptr)) return e;
    const bool hybrid = gen_weight > 0.f;
    const DiscWorkspace w = carve_disc(&ctx->plan, ws, rows, p->n_vis, p->n_hid, n_labels, hybrid ? ldv : 0);
    if (int e = check_workspace(ws, w.bytes, ws_bytes,
                                hybrid && ldv > round_up(p->n_vis, 4) ? " (ldv > round_up(n_vis, 4): the generative chain keeps v_neg at the batch's leading dimension)" : ""))
        return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hybrid) {
        // delta_gen: the label step on the same batch at the same weights, emitted and not applied (it checks k, row0, v_chain
        // before it enqueues anything, and nothing of this step has been enqueued yet)
        kurbm_cd_opts og = *o;
        og.apply = 0;
        og.delta_out = w.gen;
        og.v_planes = nullptr;
        if (int e = cd_step_f32(ctx, p, v_batch, rows, ldv, &og, 7, w.cd, w.cd_bytes, stream, nullptr, n_labels)) return e;
    }
    if (int e = class_grad_launches(ctx, p, n_labels, v_batch, rows, ldv, w, nullptr, nullptr, 0, nullptr, w.delta,
                                    hybrid ? w.gen : nullptr, gen_weight, nll_mean, st))
        return e;
    return apply_delta_f32(ctx, p, w.delta, o->lr, 7, stream, mom);
}

// ---- fine-tuning a DBN (include/kurbm.h: kurbm_backprop_layer) ---------------------------------------------------------------
// the operands of the activation-derivative site: e and x_out [rows][n_hid], delta [rows][n_hid] (it may BE e, at e's leading dimension)
static int check_site(const float* e, int lde, const float* x_out, int ldx, int rows, int n_hid, int act, const float* delta, int ldd) {
    if (int err = check_batch(e, rows, lde, n_hid, "e")) return err;
    if (int err = check_batch(x_out, rows, ldx, n_hid, "x_out")) return err;
    if (act < ACT_SIGMOID || act > ACT_LINEAR) return fail_msg(KURBM_ERR_ARG, "unknown activation %d", act);
    if (bad_matrix(delta, ldd, n_hid)) return fail_msg(KURBM_ERR_ARG, "delta: null, misaligned, ld %% 4 != 0 or ld < n_hid");
    if (delta == e && ldd != lde) return fail_msg(KURBM_ERR_ARG, "delta in place over e needs ldd == lde");
    return KURBM_OK;
}
// k_backprop_delta and k_backprop_reduce (arguments checked by the caller): delta, db_h [n_hid] and, where given, n_vis zeros at db_v
static int site_launches(const float* e, int lde, const float* x_out, int ldx, int rows, int n_hid, int act, float* delta, int ldd,
                         const BackpropWorkspace& w, float* db_h, float* db_v, int n_vis, hipStream_t st) {
    BackpropDeltaArgs d;
    memset(&d, 0, sizeof d);
    d.e = e; d.lde = lde; d.x = x_out; d.ldx = ldx; d.delta = delta; d.ldd = ldd;
    d.part = w.part; d.ld_part = w.ld_part;
    d.rows = rows; d.n_hid = n_hid; d.act = act;
    HIP_TRY(launch_backprop_delta(d, st));
    BackpropReduceArgs r;
    memset(&r, 0, sizeof r);
    r.part = w.part; r.ld_part = w.ld_part; r.ntiles = w.ntiles; r.n_hid = n_hid; r.n_vis = n_vis;
    r.db_h = db_h; r.db_v = db_v;
    HIP_TRY(launch_backprop_reduce(r, st));
    return KURBM_OK;
}
// e_in = delta.W[:n_in]^T: the linear h -> v half step on the first n_in rows of W (they are its top rows: nothing is copied), with
// `zero_bias`, n_in zeros on the device, in the bias's place -- x + 0.0f is x, so the launch and its bits are those of every other
// linear h -> v half step
static int backprop_input(kurbm_ctx* ctx, const kurbm_params* p, int n_in, const float* delta, int rows, int ldd, const float* zero_bias,
                          float* e_in, int ldei, hipStream_t st) {
    kurbm_params pp = *p;
    pp.n_vis = n_in;
    pp.b_v = const_cast<float*>(zero_bias);
    return half_step_plain(ctx, LAYOUT_HV, &pp, delta, rows, ldd, ACT_LINEAR, NOISE_NONE, nullptr, e_in, ldei, st);
}

// ---- annealed importance sampling (include/kurbm.h: kurbm_ais_run) ---------------------
// One temperature: v -> h launch (h and the softplus-difference partials), the accumulate step (it reads the (b_v - b_A).v
// partials the PREVIOUS temperature -- or the start -- left in vpart, so it runs before they are rewritten), h -> v launch
// (v and its partials).  ng_v_in: groups of vpart that hold the partials of v_in.
// ls (kurbm_ais_run_labels): the last ls->C visible units are a label block -- the h -> v launch then covers the pixel columns alone
// (they are W's top rows, and the epilogue masks the columns from N on inside a group of 16), and the label site behind it draws the
// block of v_out and leaves the block's (b_v - b_A) term as the group row behind the pixels' (w.ng_v - 1).
struct AisLabels { int C; float* prob_y; int ldp; float* u_y; };
static int ais_temperature(kurbm_ctx* ctx, const kurbm_params* p, const float* base_bias, double beta_prev, double beta, int k,
                           const float* v_in, int ldv, int rows, uint64_t chain0, uint64_t seed, const AisWorkspace& w, int ng_v_in,
                           double* logw, float* dlogw, float* h, int ldh, float* v_out, int ldvo, float* prob_h, float* u_h,
                           float* prob_v, float* u_v, hipStream_t st, const AisLabels* ls = nullptr) {
    const int n_pix = p->n_vis - (ls ? ls->C : 0);
    AisGemmArgs g;
    memset(static_cast<void*>(&g), 0, sizeof g);
    g.B0 = p->W; g.ldb = p->ldw;
    g.M = rows;
    g.nseg = 1; g.nsplit = 1;
    g.act = ACT_SIGMOID; g.noise = NOISE_BERNOULLI;
    g.base_bias = base_bias;
    g.beta_prev = (float)beta_prev; g.beta = (float)beta; g.dbeta = (float)(beta - beta_prev);
    g.one_minus_beta = (float)(1.0 - beta);
    g.ld_rowpart = w.ld_part;
    for (int layout = LAYOUT_VH; layout <= LAYOUT_HV; ++layout) {
        const bool vh = layout == LAYOUT_VH;
        g.A0 = vh ? v_in : h; g.lda = vh ? ldv : ldh;
        g.K = vh ? p->n_vis : p->n_hid; g.N = vh ? p->n_hid : n_pix;
        g.nkt = g.K / 32; g.kt_total = g.nkt; g.kt_per_split = g.nkt;
        const int cfg = pick_cfg(ctx->plan.ncu, rows, g.N, &g.grid_m, &g.grid_n, force_cfg(&ctx->plan, layout));
        g.m_fastest = (g.grid_m < g.grid_n) ? 1 : 0;
        g.bias = vh ? p->b_h : p->b_v;
        g.out_sample = vh ? h : v_out; g.out_prob = vh ? prob_h : prob_v; g.out_u = vh ? u_h : u_v; g.ldo = vh ? ldh : ldvo;
        g.rowpart = vh ? w.sppart : w.vpart;
        g.rng = make_rng(seed, chain0, vh ? KURBM_STREAM_AIS_H : KURBM_STREAM_AIS_V, (uint32_t)k);
        HIP_TRY(launch_gemm_ais(layout, cfg, g, st));
        if (vh) HIP_TRY(launch_ais_accumulate(w.sppart, w.ng_h, w.vpart, ng_v_in, w.ld_part, g.dbeta, logw, dlogw, rows, st));
        if (!vh && ls) {
            LabelSiteArgs a;
            memset(static_cast<void*>(&a), 0, sizeof a);
            a.h = h; a.ldh = ldh; a.hfmt = LS_H_F32;
            a.W = p->W; a.ldw = p->ldw; a.b_v = p->b_v;
            a.base_bias = base_bias; a.beta = g.beta; a.one_minus_beta = g.one_minus_beta;
            a.v = v_out; a.ldv = ldvo;
            a.prob = ls->prob_y; a.ldp = ls->ldp; a.prob_col0 = 0; a.out_u = ls->u_y;
            a.part = w.vpart + (size_t)(w.ng_v - 1) * w.ld_part;
            a.rows = rows; a.n_pix = n_pix; a.C = ls->C; a.n_hid = p->n_hid;
            a.rng = g.rng;
            HIP_TRY(launch_label_site(a, st));
        }
    }
    return KURBM_OK;
}

static int check_ais_common(kurbm_ctx* ctx, const kurbm_params* p, const float* base_bias, int n_chains, const void* ws,
                            size_t ws_bytes, int n_labels = 0, bool with_labels = false) {
    if (!ctx) return fail_msg(KURBM_ERR_ARG, "ctx is null");
    if (int e = check_params(p)) return e;
    if (with_labels)
        if (int e = check_labels(p, n_labels)) return e;
    if (!base_bias) return fail_msg(KURBM_ERR_ARG, "base_bias is null");
    if (n_chains <= 0) return fail_msg(KURBM_ERR_ARG, "n_chains must be positive");
    return check_workspace(ws, carve_ais(nullptr, n_chains, p->n_vis, p->n_hid, n_labels).bytes, ws_bytes);
}

static int check_betas(const double* betas, int n_betas) {
    if (!betas || n_betas < 2) return fail_msg(KURBM_ERR_ARG, "betas: null, or fewer than two temperatures");
    if (betas[0] != 0.0 || betas[n_betas - 1] != 1.0) return fail_msg(KURBM_ERR_ARG, "betas must run from 0 to 1");
    for (int k = 1; k < n_betas; ++k)
        if (!(betas[k] > betas[k - 1])) return fail_msg(KURBM_ERR_ARG, "betas must be strictly increasing (betas[%d])", k);
    return KURBM_OK;
}

// the operands of kurbm_outer_delta / kurbm_outer_partial and their workspace
static int check_outer(kurbm_ctx* ctx, const float* v_pos, const float* h_pos, const float* v_neg, const float* h_neg, int rows, int n_vis,
                       int n_hid, int ldv, int ldh, void* workspace, size_t workspace_bytes, Workspace* w) {
    if (rows <= 0 || n_vis <= 0 || n_hid <= 0) return fail_msg(KURBM_ERR_ARG, "bad shape");
    if (bad_matrix(v_pos, ldv, n_vis) || bad_matrix(v_neg, ldv, n_vis) || bad_matrix(h_pos, ldh, n_hid) ||
        bad_matrix(h_neg, ldh, n_hid))
        return fail_msg(KURBM_ERR_ARG, "operand: null, misaligned, ld %% 4 != 0 or ld < columns");
    *w = carve_f32(&ctx->plan, workspace, rows, n_vis, n_hid);
    return check_workspace(workspace, w->bytes, workspace_bytes);
}

extern "C" {

size_t kurbm_disc_workspace_bytes(kurbm_ctx* ctx, int rows, int n_vis, int n_hid, int n_labels) {
    if (!ctx || rows <= 0 || n_vis <= 0 || n_hid <= 0 || n_labels < 2 || n_labels > 64 || n_labels >= n_vis) return 0;
    return carve_disc(&ctx->plan, nullptr, rows, n_vis, n_hid, n_labels).bytes;
}

int kurbm_class_grad(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* v_batch, int rows, int ldv, float* S_y,
                     float* H_bar, int ldh, float* nll, float* delta_out, void* ws, size_t ws_bytes, kurbm_stream_t stream) {
    if (int e = check_disc(ctx, p, n_labels, v_batch, rows, ldv, ws)) return e;
    if (!delta_out || !aligned16(delta_out)) return fail_msg(KURBM_ERR_ARG, "delta_out is null or misaligned");
    if ((S_y && bad_matrix(S_y, ldh, p->n_hid)) || (H_bar && bad_matrix(H_bar, ldh, p->n_hid)))
        return fail_msg(KURBM_ERR_ARG, "S_y / H_bar: misaligned, ld %% 4 != 0 or ld < n_hid");
    if (nll && (reinterpret_cast<uintptr_t>(nll) & 3u)) return fail_msg(KURBM_ERR_ARG, "nll is misaligned");
    const DiscWorkspace w = carve_disc(&ctx->plan, ws, rows, p->n_vis, p->n_hid, n_labels);
    if (int e = check_workspace(ws, w.bytes, ws_bytes)) return e;
    // (S_y and H_bar go straight to the caller's planes, at its leading dimension: nothing else reads them)
    return class_grad_launches(ctx, p, n_labels, v_batch, rows, ldv, w, S_y, H_bar, ldh, nll, delta_out, nullptr, 0.f, nullptr,
                               static_cast<hipStream_t>(stream), knob(ctx, KN_DISC_STAGE));
}

int kurbm_disc_step(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* v_batch, int rows, int ldv,
                    const kurbm_cd_opts* opts, float gen_weight, float* nll_mean, void* ws, size_t ws_bytes, kurbm_stream_t stream,
                    const kurbm_momentum* mom) {
    return disc_step_f32(ctx, p, n_labels, v_batch, rows, ldv, opts, gen_weight, nll_mean, ws, ws_bytes, stream, mom);
}

int kurbm_disc_epoch(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* V, int n_rows, int ldv, int batch_size,
                     const kurbm_cd_opts* opts, float gen_weight, float* nll_means, void* ws, size_t ws_bytes, kurbm_stream_t stream,
                     const kurbm_momentum* mom) {
    if (int e = check_epoch(ctx, opts, n_rows, batch_size)) return e;
    kurbm_cd_opts o = *opts;
    return for_each_batch(n_rows, batch_size, [&](int lo, int rows, int step) {
        const int e = disc_step_f32(ctx, p, n_labels, V + (size_t)lo * ldv, rows, ldv, &o, gen_weight, nll_means ? nll_means + step : nullptr,
                                    ws, ws_bytes, stream, mom);
        ++o.step;
        return e;
    });
}

// ---- fine-tuning a DBN: backpropagation of log p(y | v) through its layers (include/kurbm.h: kurbm_backprop_layer) ------------
size_t kurbm_backprop_workspace_bytes(kurbm_ctx* ctx, int rows, int n_in, int n_out) {
    if (!ctx || rows <= 0 || n_in <= 0 || n_out <= 0) return 0;
    return carve_backprop(&ctx->plan, nullptr, rows, n_in, n_out).bytes;
}

int kurbm_backprop_delta(kurbm_ctx* ctx, const float* e, int lde, const float* x_out, int ldx, int rows, int n_hid, int act,
                         float* delta, int ldd, float* db_h, void* ws, size_t ws_bytes, kurbm_stream_t stream) {
    if (!ctx) return fail_msg(KURBM_ERR_ARG, "ctx is null");
    if (n_hid <= 0) return fail_msg(KURBM_ERR_ARG, "n_hid must be positive");
    if (int err = check_site(e, lde, x_out, ldx, rows, n_hid, act, delta, ldd)) return err;
    if (!db_h || (reinterpret_cast<uintptr_t>(db_h) & 3u)) return fail_msg(KURBM_ERR_ARG, "db_h is null or misaligned");
    const BackpropWorkspace w = carve_backprop(&ctx->plan, ws, rows, 1, n_hid);
    if (int err = check_workspace(ws, w.bytes, ws_bytes)) return err;
    return site_launches(e, lde, x_out, ldx, rows, n_hid, act, delta, ldd, w, db_h, nullptr, 0, static_cast<hipStream_t>(stream));
}

int kurbm_backprop_layer(kurbm_ctx* ctx, const kurbm_params* p, int act, const float* x_in, int ldin, const float* x_out, int ldout,
                         float* e, int lde, int rows, float* delta_out, float* e_in, int ldei, void* ws, size_t ws_bytes,
                         kurbm_stream_t stream) {
    if (!ctx) return fail_msg(KURBM_ERR_ARG, "ctx is null");
    if (int err = check_params(p)) return err;
    if (int err = check_batch(x_in, rows, ldin, p->n_vis, "x_in")) return err;
    if (int err = check_site(e, lde, x_out, ldout, rows, p->n_hid, act, e, lde)) return err;
    if (!delta_out || !aligned16(delta_out)) return fail_msg(KURBM_ERR_ARG, "delta_out is null or misaligned");
    if (e_in && bad_matrix(e_in, ldei, p->n_vis)) return fail_msg(KURBM_ERR_ARG, "e_in: misaligned, ld %% 4 != 0 or ld < n_vis");
    const BackpropWorkspace w = carve_backprop(&ctx->plan, ws, rows, p->n_vis, p->n_hid);
    if (int err = check_workspace(ws, w.bytes, ws_bytes)) return err;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n_vis = p->n_vis, n_hid = p->n_hid;
    const size_t nw = (size_t)n_vis * n_hid;
    // delta = e * act'(x_out) in place, db_h, and the zeros of db_v
    if (int err = site_launches(e, lde, x_out, ldout, rows, n_hid, act, e, lde, w, delta_out + nw, delta_out + nw + n_hid, n_vis, st)) return err;
    // dW = x_in^T.delta: the statistics GEMM with one segment, as class_grad_launches runs it
    const OuterPlan pl = plan_outer_one(&ctx->plan, rows, n_vis, n_hid);
    if (int err = outer_slabs(ctx, x_in, e, nullptr, nullptr, rows, n_vis, n_hid, ldin, lde, w.slab, w.slab_stride, pl, st)) return err;
    ReduceArgs a = stats_reduce_args(ctx, pl, w.slab, w.slab_stride, n_vis, n_hid, 0);
    a.delta_w = delta_out;
    HIP_TRY(launch_reduce_apply(a, st));     // (no bias work: null partial pointers)
    if (!e_in) return KURBM_OK;
    return backprop_input(ctx, p, n_vis, e, rows, lde, delta_out + nw + n_hid, e_in, ldei, st);
}

int kurbm_disc_backprop(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* v_batch, int rows, int ldv, float* delta_out,
                        float* e_in, int ldei, float* nll_mean, void* ws, size_t ws_bytes, kurbm_stream_t stream) {
    if (int err = check_disc(ctx, p, n_labels, v_batch, rows, ldv, ws)) return err;
    if (!delta_out || !aligned16(delta_out)) return fail_msg(KURBM_ERR_ARG, "delta_out is null or misaligned");
    if (e_in && bad_matrix(e_in, ldei, p->n_vis - n_labels)) return fail_msg(KURBM_ERR_ARG, "e_in: misaligned, ld %% 4 != 0 or ld < n_pix");
    if (nll_mean && (reinterpret_cast<uintptr_t>(nll_mean) & 3u)) return fail_msg(KURBM_ERR_ARG, "nll_mean is misaligned");
    const DiscWorkspace w = carve_disc(&ctx->plan, ws, rows, p->n_vis, p->n_hid, n_labels);
    if (int err = check_workspace(ws, w.bytes, ws_bytes)) return err;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int err = class_grad_launches(ctx, p, n_labels, v_batch, rows, ldv, w, nullptr, nullptr, 0, nullptr, delta_out, nullptr, 0.f, nll_mean, st))
        return err;
    if (!e_in) return KURBM_OK;
    // e = g.W[:n_pix]^T on the plane g the gradient left in the workspace; the zero bias: db_v[:n_pix] of the delta just written
    return backprop_input(ctx, p, p->n_vis - n_labels, w.g, rows, w.ldh, delta_out + (size_t)p->n_vis * p->n_hid + p->n_hid, e_in, ldei, st);
}

int kurbm_apply_delta(kurbm_ctx* ctx, const kurbm_params* p, const float* delta, float lr, int which,
                      kurbm_stream_t stream) {
    return apply_delta_f32(ctx, p, delta, lr, which, stream, nullptr);
}

int kurbm_apply_delta_mom(kurbm_ctx* ctx, const kurbm_params* p, const float* delta, float lr, int which,
                          kurbm_stream_t stream, const kurbm_momentum* mom) {
    if (int e = check_mom(mom, nullptr)) return e;
    return apply_delta_f32(ctx, p, delta, lr, which, stream, mom);
}

int kurbm_free_energy(kurbm_ctx* ctx, const kurbm_params* p, const float* v, int rows, int ldv, float* F,
                      void* workspace, size_t workspace_bytes, kurbm_stream_t stream) {
    if (!ctx || !F) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_params(p)) return e;
    if (int e = check_batch(v, rows, ldv, p->n_vis, "v")) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    GemmArgs g;
    memset(&g, 0, sizeof g);
    g.A0 = v; g.lda = ldv; g.B0 = p->W; g.ldb = p->ldw;
    g.M = rows; g.N = p->n_hid; g.K = p->n_vis;
    g.nseg = 1;
    g.nkt = g.K / 32; g.kt_total = g.nkt; g.kt_per_split = g.nkt; g.nsplit = 1;
    const int cfg = pick_cfg(ctx->plan.ncu, rows, g.N, &g.grid_m, &g.grid_n, force_cfg(&ctx->plan, LAYOUT_VH));
    g.bias = p->b_h;
    g.rowpart = static_cast<float*>(workspace);
    g.ld_rowpart = round_up(rows, 4);
    // (the row partials need less, but the contract is one size for every call on these rows: kurbm_workspace_bytes)
    size_t need = (size_t)g.grid_n * g.ld_rowpart * 4;
    const size_t query = carve_f32(&ctx->plan, nullptr, rows, p->n_vis, p->n_hid).bytes;
    if (query > need) need = query;
    if (int e = check_workspace(workspace, need, workspace_bytes)) return e;
    HIP_TRY(launch_gemm(LAYOUT_VH, cfg, EPI_SOFTPLUS, g, st));
    FinishArgs f;
    f.v = v; f.b_v = p->b_v; f.rowpart = g.rowpart; f.F = F;
    f.rows = rows; f.n_vis = p->n_vis; f.ldv = ldv; f.ncol_tiles = g.grid_n; f.ld_rowpart = g.ld_rowpart;
    HIP_TRY(launch_free_energy_finish(f, st));
    return KURBM_OK;
}

size_t kurbm_ais_workspace_bytes(kurbm_ctx* ctx, int n_chains, int n_vis, int n_hid) {
    if (!ctx || n_chains <= 0 || n_vis <= 0 || n_hid <= 0) return 0;
    return carve_ais(nullptr, n_chains, n_vis, n_hid).bytes;
}

int kurbm_ais_run(kurbm_ctx* ctx, const kurbm_params* p, const float* base_bias, const double* betas, int n_betas, int n_chains,
                  uint64_t chain0, uint64_t seed, double* logw, float* v_final, int ldv, void* ws, size_t ws_bytes,
                  kurbm_stream_t stream) {
    if (int e = check_ais_common(ctx, p, base_bias, n_chains, ws, ws_bytes)) return e;
    if (!betas || n_betas < 2) return fail_msg(KURBM_ERR_ARG, "betas: null, or fewer than two temperatures");
    if (betas[0] != 0.0 || betas[n_betas - 1] != 1.0) return fail_msg(KURBM_ERR_ARG, "betas must run from 0 to 1");
    for (int k = 1; k < n_betas; ++k)
        if (!(betas[k] > betas[k - 1])) return fail_msg(KURBM_ERR_ARG, "betas must be strictly increasing (betas[%d])", k);
    if (!logw || (reinterpret_cast<uintptr_t>(logw) & 7u)) return fail_msg(KURBM_ERR_ARG, "logw is null or misaligned");
    if (v_final && bad_matrix(v_final, ldv, p->n_vis)) return fail_msg(KURBM_ERR_ARG, "v_final: misaligned, ld %% 4 != 0 or ld < n_vis");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const AisWorkspace w = carve_ais(ws, n_chains, p->n_vis, p->n_hid);
    HIP_TRY(launch_ais_start(w.v, w.ldv, p->b_v, base_bias, w.vpart, logw, n_chains, p->n_vis, 1,
                             make_rng(seed, chain0, KURBM_STREAM_AIS_INIT, 0), st));
    for (int k = 1; k < n_betas; ++k) {
        // (the last temperature's visibles go straight to v_final; nothing reads them again)
        const bool last = k == n_betas - 1 && v_final;
        if (int e = ais_temperature(ctx, p, base_bias, betas[k - 1], betas[k], k, w.v, w.ldv, n_chains, chain0, seed, w,
                                    k == 1 ? 1 : w.ng_v, logw, nullptr, w.h, w.ldh, last ? v_final : w.v, last ? ldv : w.ldv,
                                    nullptr, nullptr, nullptr, nullptr, st))
            return e;
    }
    return KURBM_OK;
}

int kurbm_ais_step(kurbm_ctx* ctx, const kurbm_params* p, const float* base_bias, double beta_prev, double beta, int k,
                   const float* v_in, int ldv, int n_chains, uint64_t chain0, uint64_t seed, float* dlogw, float* h, int ldh,
                   float* v_out, int ldvo, float* prob_h, float* u_h, float* prob_v, float* u_v, void* ws, size_t ws_bytes,
                   kurbm_stream_t stream) {
    if (int e = check_ais_common(ctx, p, base_bias, n_chains, ws, ws_bytes)) return e;
    if (!(beta_prev >= 0.0 && beta > beta_prev && beta <= 1.0)) return fail_msg(KURBM_ERR_ARG, "need 0 <= beta_prev < beta <= 1");
    if (k < 1) return fail_msg(KURBM_ERR_ARG, "k must be >= 1");
    if (!dlogw) return fail_msg(KURBM_ERR_ARG, "dlogw is null");
    if (int e = check_batch(v_in, n_chains, ldv, p->n_vis, "v_in")) return e;
    if (int e = check_batch(h, n_chains, ldh, p->n_hid, "h")) return e;
    if (int e = check_batch(v_out, n_chains, ldvo, p->n_vis, "v_out")) return e;
    if ((prob_h && !aligned16(prob_h)) || (u_h && !aligned16(u_h)) || (prob_v && !aligned16(prob_v)) || (u_v && !aligned16(u_v)))
        return fail_msg(KURBM_ERR_ARG, "a test plane is misaligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const AisWorkspace w = carve_ais(ws, n_chains, p->n_vis, p->n_hid);
    HIP_TRY(launch_ais_start(const_cast<float*>(v_in), ldv, p->b_v, base_bias, w.vpart, nullptr, n_chains, p->n_vis, 0,
                             make_rng(seed, chain0, KURBM_STREAM_AIS_INIT, 0), st));
    return ais_temperature(ctx, p, base_bias, beta_prev, beta, k, v_in, ldv, n_chains, chain0, seed, w, 1, nullptr, dlogw, h, ldh,
                           v_out, ldvo, prob_h, u_h, prob_v, u_v, st);
}

// ---- AIS with a label block (include/kurbm.h, "free label blocks") ----------------------
size_t kurbm_ais_labels_workspace_bytes(kurbm_ctx* ctx, int n_chains, int n_vis, int n_hid, int n_labels) {
    if (!ctx || n_chains <= 0 || n_vis <= 0 || n_hid <= 0 || n_labels < 2 || n_labels > 64 || n_labels >= n_vis) return 0;
    return carve_ais(nullptr, n_chains, n_vis, n_hid, n_labels).bytes;
}

int kurbm_ais_run_labels(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* base_bias, const double* betas, int n_betas,
                         int n_chains, uint64_t chain0, uint64_t seed, double* logw, float* v_final, int ldv, void* ws, size_t ws_bytes,
                         kurbm_stream_t stream) {
    if (int e = check_ais_common(ctx, p, base_bias, n_chains, ws, ws_bytes, n_labels, true)) return e;
    if (int e = check_betas(betas, n_betas)) return e;
    if (!logw || (reinterpret_cast<uintptr_t>(logw) & 7u)) return fail_msg(KURBM_ERR_ARG, "logw is null or misaligned");
    if (v_final && bad_matrix(v_final, ldv, p->n_vis)) return fail_msg(KURBM_ERR_ARG, "v_final: misaligned, ld %% 4 != 0 or ld < n_vis");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const AisWorkspace w = carve_ais(ws, n_chains, p->n_vis, p->n_hid, n_labels);
    HIP_TRY(launch_ais_start_labels(w.v, w.ldv, p->b_v, base_bias, w.vpart, logw, n_chains, p->n_vis - n_labels, n_labels, 1,
                                    make_rng(seed, chain0, KURBM_STREAM_AIS_INIT, 0), st));
    const AisLabels ls = {n_labels, nullptr, 0, nullptr};
    for (int k = 1; k < n_betas; ++k) {
        const bool last = k == n_betas - 1 && v_final;
        if (int e = ais_temperature(ctx, p, base_bias, betas[k - 1], betas[k], k, w.v, w.ldv, n_chains, chain0, seed, w,
                                    k == 1 ? 1 : w.ng_v, logw, nullptr, w.h, w.ldh, last ? v_final : w.v, last ? ldv : w.ldv,
                                    nullptr, nullptr, nullptr, nullptr, st, &ls))
            return e;
    }
    return KURBM_OK;
}

int kurbm_ais_step_labels(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* base_bias, double beta_prev, double beta,
                          int k, const float* v_in, int ldv, int n_chains, uint64_t chain0, uint64_t seed, float* dlogw, float* h,
                          int ldh, float* v_out, int ldvo, float* prob_h, float* u_h, float* prob_v, float* u_v, float* prob_y, int ldp,
                          float* u_y, void* ws, size_t ws_bytes, kurbm_stream_t stream) {
    if (int e = check_ais_common(ctx, p, base_bias, n_chains, ws, ws_bytes, n_labels, true)) return e;
    if (!(beta_prev >= 0.0 && beta > beta_prev && beta <= 1.0)) return fail_msg(KURBM_ERR_ARG, "need 0 <= beta_prev < beta <= 1");
    if (k < 1) return fail_msg(KURBM_ERR_ARG, "k must be >= 1");
    if (!dlogw) return fail_msg(KURBM_ERR_ARG, "dlogw is null");
    if (int e = check_batch(v_in, n_chains, ldv, p->n_vis, "v_in")) return e;
    if (int e = check_batch(h, n_chains, ldh, p->n_hid, "h")) return e;
    if (int e = check_batch(v_out, n_chains, ldvo, p->n_vis, "v_out")) return e;
    if ((prob_h && !aligned16(prob_h)) || (u_h && !aligned16(u_h)) || (prob_v && !aligned16(prob_v)) || (u_v && !aligned16(u_v)))
        return fail_msg(KURBM_ERR_ARG, "a test plane is misaligned");
    if (prob_y && ldp < n_labels) return fail_msg(KURBM_ERR_ARG, "prob_y: ldp < n_labels");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const AisWorkspace w = carve_ais(ws, n_chains, p->n_vis, p->n_hid, n_labels);
    HIP_TRY(launch_ais_start_labels(const_cast<float*>(v_in), ldv, p->b_v, base_bias, w.vpart, nullptr, n_chains, p->n_vis - n_labels,
                                    n_labels, 0, make_rng(seed, chain0, KURBM_STREAM_AIS_INIT, 0), st));
    const AisLabels ls = {n_labels, prob_y, ldp, u_y};
    return ais_temperature(ctx, p, base_bias, beta_prev, beta, k, v_in, ldv, n_chains, chain0, seed, w, 1, nullptr, dlogw, h, ldh,
                           v_out, ldvo, prob_h, u_h, prob_v, u_v, st, &ls);
}

int kurbm_outer_delta(kurbm_ctx* ctx, const float* v_pos, const float* h_pos, const float* v_neg, const float* h_neg,
                      int rows, int n_vis, int n_hid, int ldv, int ldh, float* delta_w, void* workspace,
                      size_t workspace_bytes, kurbm_stream_t stream) {
    if (!ctx || !delta_w) return fail_msg(KURBM_ERR_ARG, "null argument");
    Workspace w;
    if (int e = check_outer(ctx, v_pos, h_pos, v_neg, h_neg, rows, n_vis, n_hid, ldv, ldh, workspace, workspace_bytes, &w)) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const OuterPlan pl = plan_outer(&ctx->plan, rows, n_vis, n_hid);
    if (int e = outer_slabs(ctx, v_pos, h_pos, v_neg, h_neg, rows, n_vis, n_hid, ldv, ldh, w.slab, w.slab_stride, pl, st))
        return e;
    ReduceArgs a = stats_reduce_args(ctx, pl, w.slab, w.slab_stride, n_vis, n_hid, 0);
    a.delta_w = delta_w;
    // no bias work: n_hid/n_vis bias blocks see null partial pointers and do nothing
    HIP_TRY(launch_reduce_apply(a, st));
    return KURBM_OK;
}

int kurbm_outer_partial(kurbm_ctx* ctx, const float* v_pos, const float* h_pos, const float* v_neg, const float* h_neg,
                        int rows, int n_vis, int n_hid, int ldv, int ldh, void* workspace, size_t workspace_bytes,
                        kurbm_stream_t stream) {
    if (!ctx) return fail_msg(KURBM_ERR_ARG, "null argument");
    Workspace w;
    if (int e = check_outer(ctx, v_pos, h_pos, v_neg, h_neg, rows, n_vis, n_hid, ldv, ldh, workspace, workspace_bytes, &w)) return e;
    const OuterPlan pl = plan_outer(&ctx->plan, rows, n_vis, n_hid);
    return outer_slabs(ctx, v_pos, h_pos, v_neg, h_neg, rows, n_vis, n_hid, ldv, ldh, w.slab, w.slab_stride, pl,
                       static_cast<hipStream_t>(stream));
}

}  // extern "C"
