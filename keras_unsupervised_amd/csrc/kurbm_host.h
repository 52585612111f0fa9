// kurbm_host.h -- what the host files of the C-ABI layer share (kurbm_host_ctx.hip: context, errors, knobs; kurbm_host_f32.hip:
// the fp32 path; kurbm_host_x3.hip: the bf16 / x3 path; kurbm_host_dp.hip: the data-parallel and peer steps): the context, the error
// record, the argument checks every entry point makes before it enqueues anything, and the launch sequences one file offers the others.
// Planning and workspace layouts are in kurbm_plan.h; all arithmetic is in the kernels.  No allocation, no host synchronisation.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/kurbm.h"
#include "kurbm_kernels.h"
#include "kurbm_comm.h"
#include "kurbm_plan.h"

static_assert(kurbm::DISC_TILE_ROWS == kurbm::CG_ROWS && kurbm::DISC_PART_D == kurbm::CG_PART_D, "kurbm_plan.h and kurbm_kernels.h disagree");
static_assert(kurbm::BACKPROP_TILE_ROWS == kurbm::BP_ROWS, "kurbm_plan.h and kurbm_kernels.h disagree");

constexpr size_t STATUS_BYTES = 4096;
struct kurbm_ctx {
    int device;
    kurbm::PlanCtx plan;      // the CU count and the knobs (environment, read once at creation; kurbm_ctx_set_option)
    int xcc_round_robin;      // 1: a whole-device grid puts one workgroup of every octet (b / 8) on each of eight XCDs (probed at creation)
    unsigned xcc_map;         // the XCDs of workgroups 0 .. 7 of the probe launch, a nibble each (diagnostic)
    unsigned* status;   // device word, sticky: kurbm_ctx_status, in front of the only device memory the library owns (STATUS_BYTES: behind
                        // the status word the grid barrier of kurbm_cd_step_small -- words 64 .. 223: eight per-XCD arrival counters, the
                        // grid's counter, the generation word, one 64-byte line each)
};

namespace kurbm {

// (fail_msg, kurbm_comm.h: records the message kurbm_last_error() returns and passes the code through)
#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail_msg(KURBM_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

static inline int knob(const kurbm_ctx* ctx, int which) { return ctx->plan.knob[which]; }
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline bool bad_matrix(const void* p, int ld, int cols) { return !p || !aligned16(p) || ld % 4 != 0 || ld < cols; }

// ---- argument checks: everything is refused before anything is enqueued ------------------------------------------------------
static inline int check_params(const kurbm_params* p) {
    if (!p) return fail_msg(KURBM_ERR_ARG, "params is null");
    if (p->n_vis <= 0 || p->n_hid <= 0) return fail_msg(KURBM_ERR_ARG, "n_vis/n_hid must be positive");
    if (bad_matrix(p->W, p->ldw, p->n_hid)) return fail_msg(KURBM_ERR_ARG, "W: null, misaligned, or ldw %% 4 != 0 / ldw < n_hid");
    if (!p->b_h || !p->b_v) return fail_msg(KURBM_ERR_ARG, "bias pointer is null");
    return KURBM_OK;
}
// the batch operand: `rows` rows of `cols` floats at leading dimension ld
static inline int check_batch(const float* v, int rows, int ld, int cols, const char* name = "v_batch") {
    if (rows <= 0) return fail_msg(KURBM_ERR_ARG, "rows must be positive");
    if (bad_matrix(v, ld, cols)) return fail_msg(KURBM_ERR_ARG, "%s: null, misaligned, ld %% 4 != 0 or ld < %d columns", name, cols);
    return KURBM_OK;
}
static inline int check_mode(int mode) {
    if (mode != KURBM_MODE_VISIBLE_BERNOULLI && mode != KURBM_MODE_VISIBLE_GAUSSIAN) return fail_msg(KURBM_ERR_ARG, "unknown mode %d", mode);
    return KURBM_OK;
}
// the fields of kurbm_cd_opts every step reads (with_k: the entry point runs CD-k; with_row0: it has rows to draw for)
static inline int check_opts(const kurbm_cd_opts* o, bool with_k = true, bool with_row0 = true) {
    if (with_k && (o->k < 1 || o->k > 15)) return fail_msg(KURBM_ERR_ARG, "k must be in [1, 15]");
    if (int e = check_mode(o->mode)) return e;
    if (with_row0 && (o->row0 & 3)) return fail_msg(KURBM_ERR_ARG, "row0 must be a multiple of 4");
    return KURBM_OK;
}
// a caller-sized buffer ("workspace", "mirror", "planes"): present, aligned, large enough
static inline int check_buffer(const char* name, const void* buf, size_t need, size_t got, const char* hint = "") {
    if (!buf || !aligned16(buf)) return fail_msg(KURBM_ERR_ARG, "%s is null or misaligned", name);
    if (need > got) return fail_msg(KURBM_ERR_WORKSPACE, "%s too small: need %zu bytes, got %zu%s", name, need, got, hint);
    return KURBM_OK;
}
static inline int check_workspace(const void* ws, size_t need, size_t got, const char* hint = "") { return check_buffer("workspace", ws, need, got, hint); }
static inline int check_v_pieces(int v_pieces) {
    if (v_pieces != 1 && v_pieces != 3 && v_pieces != (1 | KURBM_V_BINARY)) return fail_msg(KURBM_ERR_ARG, "v_pieces must be 1, 1 | KURBM_V_BINARY or 3");
    return KURBM_OK;
}
static inline int check_labels(const kurbm_params* p, int n_labels) {
    if (n_labels < 2 || n_labels > 64) return fail_msg(KURBM_ERR_ARG, "n_labels must be in [2, 64], got %d", n_labels);
    if (n_labels >= p->n_vis) return fail_msg(KURBM_ERR_ARG, "n_labels = %d leaves no pixel among %d visible units", n_labels, p->n_vis);
    return KURBM_OK;
}
// Momentum / weight decay of the *_mom entry points (include/kurbm.h)
static inline int check_mom(const kurbm_momentum* m, const kurbm_cd_opts* o) {
    if (!m || !m->vel) return fail_msg(KURBM_ERR_ARG, "momentum block or its velocity buffer is null");
    if (!aligned16(m->vel)) return fail_msg(KURBM_ERR_ARG, "the velocity buffer is not 16-byte aligned");
    if (!(m->momentum >= 0.f && m->momentum < 1.f)) return fail_msg(KURBM_ERR_ARG, "momentum must be in [0, 1), got %g", (double)m->momentum);
    if (!(m->weight_decay >= 0.f)) return fail_msg(KURBM_ERR_ARG, "weight_decay must be >= 0, got %g", (double)m->weight_decay);
    if (o && !o->apply) return fail_msg(KURBM_ERR_ARG, "the momentum entry points apply the update in place: apply = 1");
    return KURBM_OK;
}
// ... as the kernels take it: the three velocities of the packed buffer, W's from visible row m_lo on.  A null block gives the
// launchers' null: the ordinary kernels.
struct MomOpt {
    MomArgs args;
    bool on;
    const MomArgs* ptr() const { return on ? &args : nullptr; }
};
static inline MomOpt make_mom(const kurbm_params* p, const kurbm_momentum* m, int m_lo = 0) {
    MomOpt mo;
    mo.on = m != nullptr;
    if (!m) return mo;
    const size_t nw = (size_t)p->n_vis * p->n_hid;
    mo.args.mu = m->momentum; mo.args.decay = m->weight_decay;
    mo.args.vel_w = m->vel + (size_t)m_lo * p->n_hid; mo.args.vel_bh = m->vel + nw; mo.args.vel_bv = m->vel + nw + p->n_hid;
    return mo;
}

// The hidden and visible activations and the visible noise of a mode: sigmoid / sigmoid / Bernoulli, or for Gaussian visibles
// relu / linear / Gaussian (rbm.py:47, :53 against :59, :64-65); hidden units are always sampled as Bernoulli
struct ModeActs { int act_h, act_v, noise_v; };
static inline ModeActs mode_acts(bool gauss) {
    return {gauss ? ACT_RELU : ACT_SIGMOID, gauss ? ACT_LINEAR : ACT_SIGMOID, gauss ? NOISE_GAUSSIAN : NOISE_BERNOULLI};
}

// Where the sums of a CD step go (launch_reduce_apply, launch_reduce_apply_split): lr * sums into the parameters `which` selects
// when the step applies, and / or the sums themselves into the packed delta dW | db_h | db_v (dW from visible row m_lo on)
static inline void reduce_targets(ReduceArgs& a, const kurbm_params* p, const kurbm_cd_opts* o, int which, int m_lo = 0) {
    const bool ap = o->apply != 0;
    const size_t nw = (size_t)p->n_vis * p->n_hid;
    a.lr = o->lr;
    a.W = (ap && (which & 1)) ? p->W : nullptr;
    a.b_h = (ap && (which & 2)) ? p->b_h : nullptr;
    a.b_v = (ap && (which & 4)) ? p->b_v : nullptr;
    a.delta_w = o->delta_out ? o->delta_out + (size_t)m_lo * p->n_hid : nullptr;
    a.delta_bh = o->delta_out ? o->delta_out + nw : nullptr;
    a.delta_bv = o->delta_out ? o->delta_out + nw + p->n_hid : nullptr;
}

static inline RngArgs make_rng(uint64_t seed, uint64_t row0, uint32_t stream_id, uint32_t step) {
    RngArgs r;
    r.seed_lo = (uint32_t)(seed & 0xFFFFFFFFu);
    r.seed_hi = (uint32_t)(seed >> 32);
    r.stream_id = stream_id;
    r.step = step;
    r.row0 = row0;
    return r;
}
static inline RngArgs make_rng(const kurbm_rng* rng) { return make_rng(rng->seed, rng->row0, rng->stream_id, rng->step); }

// ---- an epoch: `step(lo, rows, index)` for each batch of n_rows rows; returns the number of steps or the first error ---------
static inline int check_epoch(const void* ctx, const kurbm_cd_opts* opts, int n_rows, int batch_size) {
    if (!ctx || !opts) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (n_rows < 0 || batch_size <= 0) return fail_msg(KURBM_ERR_ARG, "bad row count / batch size");
    return KURBM_OK;
}
template <class Step> static int for_each_batch(int n_rows, int batch_size, Step step) {
    int steps = 0;
    for (int lo = 0; lo < n_rows; lo += batch_size, ++steps)
        if (int e = step(lo, (n_rows - lo < batch_size) ? n_rows - lo : batch_size, steps)) return e;
    return steps;
}

// ---- launch sequences one host file offers the others (arguments checked as their comments say) --------------------------------
// kurbm_host_f32.hip: W, b_h, b_v += lr * packed delta (kurbm_apply_delta; mom nullable)
int apply_delta_f32(kurbm_ctx* ctx, const kurbm_params* p, const float* delta, float lr, int which, kurbm_stream_t stream,
                    const kurbm_momentum* mom);
// kurbm_host_x3.hip.  check_cd_args: every argument check of a bf16 / x3 CD step; cd_step_any: the step, one stage of it, its chain
// (only = 8) or the statistics of visible rows [m_lo, m_hi) (only = 7); apply_delta_rows: rows [m_lo, m_hi) of W and its mirror
// (with `bias`, the biases too) += lr * packed delta, one launch; mirror_refresh_any: both weight mirrors from the fp32 master
int check_cd_args(kurbm_ctx* ctx, int pieces, int v_pieces, const kurbm_params* p, const void* mirror, size_t mirror_bytes,
                  const float* v_batch, int rows, int ldv, const kurbm_cd_opts* o, const void* workspace, size_t workspace_bytes,
                  bool zero_rows_ok);
int cd_step_any(kurbm_ctx* ctx, int pieces, int v_pieces, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                const float* v_batch, int rows, int ldv, const kurbm_cd_opts* o, int which, void* workspace, size_t workspace_bytes,
                kurbm_stream_t stream, int only = -1, int m_lo = 0, int m_hi = -1, const kurbm_momentum* mom = nullptr);
int apply_delta_rows(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, int pieces, const float* delta,
                     float lr, int which, int m_lo, int m_hi, bool bias, hipStream_t st, const kurbm_momentum* mom = nullptr);
int mirror_refresh_any(kurbm_ctx* ctx, int pieces, const kurbm_params* p, void* mirror, size_t mirror_bytes, kurbm_stream_t stream);

}  // namespace kurbm
