/*
 * kurbm.h -- C ABI of the MI355X (gfx950) RBM / DBN contrastive-divergence engine.
 *
 * This is the drop-in boundary for the hot path of tonandr/keras_unsupervised's
 * ku/ebm package.  The reference has no FFI of its own: its narrowest seam is the set of
 * seven K.function closures an RBM object owns (reference ku/ebm/rbm.py:48, :54, :76,
 * :127, :129, :132, :137) plus its three variables (rbm.py:30-40).  Each entry point
 * below cites the closure(s) it replaces.  The Python classes in
 * keras_unsupervised_amd/ebm bind these with ctypes (see INTEGRATION.md for the stub a
 * reference maintainer would add).
 *
 * Conventions (all entry points)
 *   - every pointer named v/h/W/b_*, out_*, delta, workspace is a DEVICE pointer into
 *     caller-owned memory; the library never allocates or frees device memory and never
 *     synchronises with the host;
 *   - matrices are row-major fp32 [rows, ld]; ld is in floats, ld % 4 == 0, ld >= columns;
 *     base addresses are 16-byte aligned.  Columns [cols, ld) are padding: inputs may hold
 *     anything there, outputs are left untouched there.  These promises -- nothing written outside a caller's buffer, padding
 *     neither written nor let into a result, a buffer below its size query refused before anything is enqueued -- are tested:
 *     tests/test_gpu_guard_bands.py runs every entry point on guarded, NaN-padded, wide-ld buffers (tests/guarded.py);
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream);
 *   - return value: 0 = KURBM_OK, < 0 = error; kurbm_last_error() returns a thread-local
 *     message for the last failing call on this thread;
 *   - a kurbm_ctx belongs to one device and must not be used from two threads at once.
 *
 * Random numbers: Philox4x32-10, key = (seed_lo, seed_hi),
 *   counter = (col, (row0 + row) >> 2, stream_id, step), word (row0 + row) & 3,
 *   u = bitcast_f32((word & 0x7FFFFF) | 0x3F800000) - 1.0f.   row0 % 4 == 0 is required.
 *   Normals (Gaussian visible units): Box-Muller over the planes stream_id and
 *   stream_id | 0x80000000.  The CPU statement of the same contract is oracle/philox.py.
 */
#ifndef KURBM_H
#define KURBM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KURBM_ABI_VERSION 5

typedef struct kurbm_ctx kurbm_ctx;
typedef struct kurbm_comm kurbm_comm; /* one RCCL communicator + the library's comm stream and events, per GPU */
typedef void* kurbm_stream_t; /* hipStream_t */

enum {
    KURBM_OK = 0,
    KURBM_ERR_ARG = -1,         /* bad pointer / shape / alignment */
    KURBM_ERR_HIP = -2,         /* a HIP runtime call failed */
    KURBM_ERR_UNSUPPORTED = -3, /* valid request this build does not implement */
    KURBM_ERR_WORKSPACE = -4,   /* workspace too small */
    KURBM_ERR_COMM = -5         /* RCCL missing or an RCCL call failed */
};

/* Activation applied to the pre-activation x = in.W(+T) + bias. */
enum {
    KURBM_ACT_SIGMOID = 0, /* Bernoulli units: rbm.py:47, :53, :124 */
    KURBM_ACT_RELU = 1,    /* Gaussian-mode hidden threshold: rbm.py:59, :86 */
    KURBM_ACT_LINEAR = 2   /* Gaussian visible mean: rbm.py:64-65, :143 */
};

/* What is drawn from the activated value p. */
enum {
    KURBM_NOISE_NONE = 0,      /* no draw: only out_prob is written (h_neg, rbm.py:124) */
    KURBM_NOISE_BERNOULLI = 1, /* out_sample = (u < p) ? 1 : 0   (rbm.py:46-47, :121-123) */
    KURBM_NOISE_GAUSSIAN = 2   /* out_sample = p + z, z ~ N(0,1) (rbm.py:64-66, :143-144) */
};

/* RBM.mode of the reference (rbm.py:14-16). */
enum { KURBM_MODE_VISIBLE_BERNOULLI = 0, KURBM_MODE_VISIBLE_GAUSSIAN = 1 };

/* The three variables of an RBM (rbm.py:30-40), resident on the device. */
typedef struct {
    int32_t n_vis;  /* rows of W */
    int32_t n_hid;  /* columns of W */
    int32_t ldw;    /* leading dimension of W in floats */
    int32_t _pad;
    float* W;       /* [n_vis, ldw]  rbm_weight      rbm.py:30-33 */
    float* b_h;     /* [n_hid]       rbm_hidden_bias rbm.py:34-37 */
    float* b_v;     /* [n_vis]       visible_bias    rbm.py:38-40 */
} kurbm_params;

/* One sampling site of the RNG contract. */
typedef struct {
    uint64_t seed;
    uint64_t row0;      /* global index of the first row; multiple of 4 */
    uint32_t stream_id;
    uint32_t step;
} kurbm_rng;

/* Options of one contrastive-divergence parameter update. */
typedef struct {
    int32_t k;          /* Gibbs iterations (reference: 1)                          */
    int32_t mode;       /* KURBM_MODE_*                                             */
    float lr;           /* hps['lr'], applied to batch SUMS (rbm.py:128,130,133)    */
    int32_t apply;      /* 1: W,b_h,b_v += lr*delta in place; 0: only emit delta    */
    float* delta_out;   /* nullable; packed [n_vis*n_hid | n_hid | n_vis] fp32 sums */
    float* v_chain;     /* nullable; persistent chain [rows, ldv], read then overwritten
                           with v_neg (extension; absent from the reference)         */
    uint64_t seed;
    uint64_t row0;      /* global row offset of this shard (data parallel); % 4 == 0 */
    uint32_t step;      /* parameter-update counter                                  */
    uint32_t chain;     /* chain id: stream ids are chain*64 + {2t, 2t-1}            */
    const void* v_planes;      /* nullable; x3 only: the bf16 planes kurbm_x3_convert_rows made of exactly the rows of
                                  v_batch -- the step then skips its own conversion (the data matrix is static for
                                  a whole fit(): rbm.py:211 slices the same V every epoch)               */
    uint64_t v_planes_stride;  /* kurbm_cd_epoch_x3: bytes between the planes of consecutive batches   */
} kurbm_cd_opts;

/* ---- context ------------------------------------------------------------------- */
int kurbm_abi_version(void);
const char* kurbm_last_error(void);
int kurbm_ctx_create(int device, kurbm_ctx** out);
void kurbm_ctx_destroy(kurbm_ctx* ctx);
/* Tuning / test hook: the library reads its experiment knobs (the KURBM_* variables listed in DESIGN.md) from the
 * environment once, in kurbm_ctx_create; this sets one of them (by its environment name, e.g. "KURBM_X3_TALL") on a
 * live context.  -1 = automatic where a knob has an automatic setting.  No production caller needs it. */
int kurbm_ctx_set_option(kurbm_ctx* ctx, const char* name, int value);
/* Sticky status bits of the context's kernels, read back from the device (THIS call synchronises with the device; the
 * others never do) and cleared.  Every device-side wait in this library is bounded; a wait that runs into its bound sets a bit
 * here and SKIPS its work instead of hanging the GPU.  Bit 1: the peer exchange (kurbm_peer_*) gave up waiting for a rank's flag.
 * Bit 2: a barrier of kurbm_cd_step_small timed out -- its grid was not resident (a CU mask, a device shared with a kernel
 * that never ends).  0 in every run this build has seen; the host classes read it at the end of every fit() and raise. */
int kurbm_ctx_status(kurbm_ctx* ctx, int* bits);

/* ---- RNG test hook: out[r, c] = u(row0 + r, c) under the contract above -------- */
int kurbm_philox_uniform(kurbm_ctx* ctx, float* out, int rows, int cols, int ld,
                         const kurbm_rng* rng, kurbm_stream_t stream);

/*
 * visible -> hidden half step.   Replaces transform_func (rbm.py:46-48 / :58-60), the body
 * of RBM.call (rbm.py:80-86) and, with noise = NONE, the h_neg expression (rbm.py:124).
 *   x = v.W + b_h ; p = act(x) ; out_prob = p (nullable) ; out_sample per `noise` (nullable)
 * ONE kernel launch: MFMA GEMM + fused bias / activation / Philox draw epilogue.
 */
int kurbm_half_step_vh(kurbm_ctx* ctx, const kurbm_params* p, const float* v, int rows, int ldv,
                       int act, int noise, const kurbm_rng* rng,
                       float* out_sample, float* out_prob, int ldh, kurbm_stream_t stream);

/*
 * hidden -> visible half step.   Replaces inv_transform_func (rbm.py:52-54 / :64-67) and
 * the v_neg expression of the CD graph (rbm.py:121-123 / :143-144).  W is read as stored
 * (never transposed in memory):   x = h.W^T + b_v.
 */
int kurbm_half_step_hv(kurbm_ctx* ctx, const kurbm_params* p, const float* h, int rows, int ldh,
                       int act, int noise, const kurbm_rng* rng,
                       float* out_sample, float* out_prob, int ldv, kurbm_stream_t stream);

/* Test hooks: the same launches, additionally writing the uniforms that were compared
 * against the probabilities (out_u, nullable, same shape/ld as the outputs). */
int kurbm_half_step_vh_dbg(kurbm_ctx* ctx, const kurbm_params* p, const float* v, int rows, int ldv,
                           int act, int noise, const kurbm_rng* rng, float* out_sample,
                           float* out_prob, float* out_u, int ldh, kurbm_stream_t stream);
int kurbm_half_step_hv_dbg(kurbm_ctx* ctx, const kurbm_params* p, const float* h, int rows, int ldh,
                           int act, int noise, const kurbm_rng* rng, float* out_sample,
                           float* out_prob, float* out_u, int ldv, kurbm_stream_t stream);

/* Bytes of scratch the fp32 entry points (kurbm_cd_step, kurbm_cd_epoch, kurbm_free_energy, kurbm_outer_delta, the small path)
 * need for batches of <= rows; 0 for a non-positive shape.  Every one of them refuses a smaller workspace (KURBM_ERR_WORKSPACE).
 * One addition: kurbm_cd_step / kurbm_cd_epoch (and their _mom twins) keep the negative visibles in the workspace at the leading
 * dimension of the batch, so a batch with ldv > round_up(n_vis, 4) (a column window of a wider matrix) needs
 *     up256(rows * ldv * 4) - up256(rows * round_up(n_vis, 4) * 4)      (up256: rounded up to a multiple of 256)
 * bytes more than this query reports, and is refused without them. */
size_t kurbm_workspace_bytes(kurbm_ctx* ctx, int rows, int n_vis, int n_hid, int k);

/*
 * One CD-k parameter update from one Gibbs chain.   Replaces rbm_weight_update_func,
 * hidden_bias_update_func and visible_bias_update_func (rbm.py:125-134) evaluated on ONE
 * chain (update_mode "fused"); `chain` selects an independent chain so the host can also
 * replay the reference's three-chain sequence (rbm.py:214-216).
 * Launch sequence: half_vh(sample) ; k x [half_hv(sample) ; half_vh] ; outer-product
 * split-K GEMM over [v_pos ; -v_neg]^T.[h_pos ; h_neg] ; reduce (+ apply).
 * `which` is a bit mask of what `apply` touches: 1 = W, 2 = b_h, 4 = b_v (7 = all).
 */
int kurbm_cd_step(kurbm_ctx* ctx, const kurbm_params* p, const float* v_batch, int rows, int ldv,
                  const kurbm_cd_opts* opts, int which, void* workspace, size_t workspace_bytes,
                  kurbm_stream_t stream);

/*
 * One pass of the training loop over a resident data matrix: for each contiguous batch, in order,
 * remainder last (rbm.py:110-111, :163, :211, :218), one kurbm_cd_step with opts->step advancing by
 * one per batch.  Replaces the Python-level batch loop of RBM.fit for update_mode "fused" when no
 * per-step score is requested; identical launches, no host round trip per step.  A persistent
 * chain (opts->v_chain) must hold batch_size rows.  Returns the number of steps taken (>= 0) or an
 * error code (< 0).
 */
int kurbm_cd_epoch(kurbm_ctx* ctx, const kurbm_params* p, const float* V, int n_rows, int ldv, int batch_size,
                   const kurbm_cd_opts* opts, void* workspace, size_t workspace_bytes, kurbm_stream_t stream);

/* params += lr * delta for a packed delta (after the data-parallel all-reduce). */
int kurbm_apply_delta(kurbm_ctx* ctx, const kurbm_params* p, const float* delta, float lr,
                      int which, kurbm_stream_t stream);

/*
 * Free energy F(v) = -(v.b_v + sum_j softplus((v.W + b_h)_j)).   Replaces
 * free_energy_func (rbm.py:73-76), with the overflow-free softplus.
 */
int kurbm_free_energy(kurbm_ctx* ctx, const kurbm_params* p, const float* v, int rows, int ldv,
                      float* F, void* workspace, size_t workspace_bytes, kurbm_stream_t stream);

/*
 * Sufficient-statistics GEMM alone (bench / test hook for the dominant kernel):
 *   delta[0 : n_vis*n_hid] = v_pos^T.h_pos - v_neg^T.h_neg   (dense, ld = n_hid)
 */
int kurbm_outer_delta(kurbm_ctx* ctx, const float* v_pos, const float* h_pos, const float* v_neg,
                      const float* h_neg, int rows, int n_vis, int n_hid, int ldv, int ldh,
                      float* delta_w, void* workspace, size_t workspace_bytes,
                      kurbm_stream_t stream);

/*
 * The split-K slab GEMM of kurbm_outer_delta WITHOUT the slab reduction (measurement hook: this
 * is the dominant kernel of a CD step, timed alone for the roofline line of bench.py).  The
 * partial sums stay in `workspace`.
 */
int kurbm_outer_partial(kurbm_ctx* ctx, const float* v_pos, const float* h_pos, const float* v_neg,
                        const float* h_neg, int rows, int n_vis, int n_hid, int ldv, int ldh,
                        void* workspace, size_t workspace_bytes, kurbm_stream_t stream);

/* ---- bf16 storage / fp32 accumulate (extension; BASELINE.json config 5) --------------------
 *
 * The fp32 parameters of kurbm_params stay authoritative.  A MIRROR buffer (caller-owned device
 * memory, kurbm_bf16_mirror_bytes) holds their bf16 images in both orientations; it must be
 * refreshed (kurbm_bf16_mirror_refresh) whenever the caller writes the fp32 weights, and is kept in
 * sync by kurbm_cd_step_bf16 itself.  Inputs and outputs of these entry points are fp32 exactly as in
 * the fp32 API; only the matrix products run on bf16 operands (weights, data and probabilities
 * rounded to nearest even; 0/1 samples are exact), accumulated in fp32.
 */
size_t kurbm_bf16_mirror_bytes(kurbm_ctx* ctx, int n_vis, int n_hid);
int kurbm_bf16_mirror_refresh(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                              kurbm_stream_t stream);
size_t kurbm_bf16_workspace_bytes(kurbm_ctx* ctx, int rows, int n_vis, int n_hid, int k);

/* Same contract as kurbm_cd_step, products in bf16. */
int kurbm_cd_step_bf16(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                       const float* v_batch, int rows, int ldv, const kurbm_cd_opts* opts, int which,
                       void* workspace, size_t workspace_bytes, kurbm_stream_t stream);

/* One half step with bf16 products (test hook): dir 0 = v->h, 1 = h->v; fp32 in, fp32 planes out. */
int kurbm_half_step_bf16(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, int dir,
                         const float* in, int rows, int ld_in, int act, int noise, const kurbm_rng* rng,
                         float* out_sample, float* out_prob, float* out_u, int ld_out,
                         void* workspace, size_t workspace_bytes, kurbm_stream_t stream);

/* ---- x3: fp32 values as exact bf16 triples on the bf16 matrix cores (extension) ---------------
 *
 * gfx950 multiplies bf16 operands 16x faster than fp32 ones (v_mfma_f32_16x16x32_bf16 vs
 * v_mfma_f32_16x16x4_f32), and every fp32 value is EXACTLY the sum of three bf16 values
 * (x = hi + mid + lo, round-to-nearest at each stage).  The x3 entry points keep fp32 storage and
 * fp32 accumulation, but carry each real-valued GEMM operand as its three pieces and run one
 * k-segment of the product per pair of pieces; 0/1 samples (h_pos, v_neg, the hidden and visible
 * states of a Bernoulli chain) are a single exact piece.  Products of pieces are exact in fp32, so the
 * result differs from an fp32 GEMM only in the order of the fp32 additions.  Same reference
 * operations as the fp32 entry points (rbm.py:46-47, :121-134), both visible modes: with
 * MODE_VISIBLE_GAUSSIAN (rbm.py:55-67, :139-159) the negative visibles are real-valued and travel as three
 * pieces too (row-major for the next half step, transposed for the statistics).
 *
 * v_pieces: 1 promises that every element of v_batch (and of opts->v_chain) is exactly a bf16
 * value, which 0/1 data is (check with kurbm_bf16_exact); 3 splits the batch as well.  When both
 * operands of a product are split, the three pairs of pieces below 2^-24 of the product are left out.
 * 1 | KURBM_V_BINARY additionally promises that every element of v_batch (and of opts->v_chain) is 0.0 or 1.0 (bit 1 of
 * kurbm_bf16_exact's flag clear).  The library then keeps the data planes, like those of its own 0/1 samples, as bytes
 * instead of bf16 (half the traffic of the A operand of a half step), and runs the positive statistics v_pos^T h_pos, a
 * 0/1 x 0/1 product, on the fp8 matrix cores (twice the bf16 rate).  Both are exact: the operands are 0 or 1, the
 * accumulation is fp32.  A window of resident planes (kurbm_x3_convert_rows) must be made and used with the same
 * v_pieces value.
 * The mirror holds the pieces of W in both orientations and follows the rules of the bf16 mirror.
 */
#define KURBM_V_BINARY 0x10
size_t kurbm_x3_mirror_bytes(kurbm_ctx* ctx, int n_vis, int n_hid);
int kurbm_x3_mirror_refresh(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                            kurbm_stream_t stream);
size_t kurbm_x3_workspace_bytes(kurbm_ctx* ctx, int rows, int n_vis, int n_hid, int k, int v_pieces);

/* Same contract as kurbm_cd_step. */
int kurbm_cd_step_x3(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                     const float* v_batch, int v_pieces, int rows, int ldv, const kurbm_cd_opts* opts,
                     int which, void* workspace, size_t workspace_bytes, kurbm_stream_t stream);

/*
 * Measurement hook: ONE launch of the kurbm_cd_step_x3 sequence, on the planes a previous complete
 * step left in `workspace` (same arguments as that step).  stage: 0 v_pos -> bf16 pieces, 1 h_pos half
 * step, 2 v_neg half step(s), 3 h_neg half step, 4 statistics GEMM, 5 slab reduction + parameter
 * update + mirror refresh, 6 mirror refresh alone.  bench.py times the kernels of a step with it.
 */
int kurbm_cd_step_x3_stage(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                           const float* v_batch, int v_pieces, int rows, int ldv, const kurbm_cd_opts* opts,
                           int which, int stage, void* workspace, size_t workspace_bytes,
                           kurbm_stream_t stream);

/* Test hook: the planes the last complete kurbm_cd_step_x3 (same rows, v_pieces, opts->mode; CD-1, no persistent chain) left
 * in `workspace`, decoded to fp32 [rows][units] -- bytes (0x40 = one, k-permuted), fp8 (0x38 = one), bf16, or the sum of
 * three bf16 pieces; transposed planes are transposed back, the negated h_neg plane is un-negated.  The tests compare them
 * with the states the half-step hooks return for the same counters, i.e. with the oracle. */
enum { KURBM_PLANE_H_POS = 0, KURBM_PLANE_H_POS_T = 1, KURBM_PLANE_V_NEG = 2, KURBM_PLANE_V_NEG_T = 3, KURBM_PLANE_H_NEG_T = 4 };
int kurbm_x3_dump_plane(kurbm_ctx* ctx, int which, int rows, int n_vis, int n_hid, int v_pieces, int mode,
                        const void* workspace, size_t workspace_bytes, float* out, int ld_out, kurbm_stream_t stream);

/* The per-step score of fit(verbose = 1), rbm.py:225-233, on the x3 path in ONE call with nothing returned to the host:
 * fe = F(v_batch); v' = a one-step reconstruction of v_batch (fresh chain: opts->chain, sites 0 and 1, opts->step, opts->seed,
 * opts->row0, opts->mode; opts->v_planes as for a step); fe' = F(v'); *score = mean |fe - fe'| (device float, 16-byte
 * aligned); F (nullable, device [2 * rows]) receives fe then fe'.  Workspace as for kurbm_cd_step_x3 on the same rows; the
 * caller reads *score back when it wants to print it (the reference prints every step: rbm.py:234). */
int kurbm_score_x3(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v_batch,
                   int v_pieces, int rows, int ldv, const kurbm_cd_opts* opts, float* score, float* F, void* workspace,
                   size_t workspace_bytes, kurbm_stream_t stream);

/* kurbm_free_energy on the x3 path (rbm.py:73-76): workspace of kurbm_x3_workspace_bytes of the same rows and v_pieces
 * (it holds the bf16 pieces of v and one float per row and 128-column tile; a smaller one is refused). */
int kurbm_free_energy_x3(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v,
                         int v_pieces, int rows, int ldv, float* F, void* workspace, size_t workspace_bytes,
                         kurbm_stream_t stream);

/* kurbm_cd_epoch on the x3 path: every batch of an epoch in one call (fused updates; returns the number of steps).
 * All work is ordered on `stream`.  With opts->v_planes the planes of batch t are read at v_planes + t * v_planes_stride. */
int kurbm_cd_epoch_x3(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* V,
                      int v_pieces, int n_rows, int ldv, int batch_size, const kurbm_cd_opts* opts,
                      void* workspace, size_t workspace_bytes, kurbm_stream_t stream);

/*
 * The data-parallel x3 step in pieces, so that the all-reduce of the first rows of dW can run while the rest is
 * still being computed:  kurbm_cd_chain_x3 = the chain alone (v_pos -> bf16, the three half steps; leaves the
 * states in `workspace`);  kurbm_x3_stats_rows = the statistics of visible rows [m_lo, m_hi) of that chain into
 * opts->delta_out (packed [dW | db_h | db_v]; rows m_lo .. m_hi-1 of dW, and with m_hi == n_vis also db_h and
 * db_v).  m_lo a multiple of 128; opts->apply = 0.  Calling it for [0, m) and [m, n_vis) gives the delta of
 * kurbm_cd_step_x3(apply = 0) up to the order of the fp32 additions (the split-K slicing differs).
 */
int kurbm_cd_chain_x3(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v_batch,
                      int v_pieces, int rows, int ldv, const kurbm_cd_opts* opts, void* workspace,
                      size_t workspace_bytes, kurbm_stream_t stream);
int kurbm_x3_stats_rows(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                        const float* v_batch, int v_pieces, int rows, int ldv, const kurbm_cd_opts* opts, int m_lo,
                        int m_hi, void* workspace, size_t workspace_bytes, kurbm_stream_t stream);

/* kurbm_apply_delta for the x3 path (data-parallel step): W, b_h, b_v += lr * delta AND the mirror's weight
 * pieces rewritten, in one launch. */
int kurbm_x3_apply_delta(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                         const float* delta, float lr, int which, kurbm_stream_t stream);

/*
 * Resident data planes.  RBM.fit slices the same matrix V every epoch (rbm.py:113, :211), so its bf16 images -- the pieces
 * of the rows row-major and transposed, and their column sums per 64-row band -- are made ONCE per window of rows and a
 * step given opts->v_planes reads them instead of converting the window again.  `planes` is caller-owned device memory of
 * kurbm_x3_planes_bytes(rows) bytes per window; its layout follows `rows` (a remainder batch has its own) and v_pieces:
 * with 1 | KURBM_V_BINARY the row-major plane holds bytes and the transposed one fp8 (see above), so the steps that read a
 * window must pass the v_pieces it was made with, under the same KURBM_X3_BYTES / KURBM_X3_F8POS settings of the context.
 */
size_t kurbm_x3_planes_bytes(kurbm_ctx* ctx, int rows, int n_vis, int v_pieces);
int kurbm_x3_convert_rows(kurbm_ctx* ctx, const float* v, int rows, int ldv, int n_vis, int v_pieces, void* planes,
                          size_t planes_bytes, kurbm_stream_t stream);

/* One half step on the x3 path (transform / test hook): dir 0 = v->h, 1 = h->v.
 * in_pieces describes `in` as v_pieces describes a batch: 3 splits any fp32 input into its three pieces; 1 promises that every
 * element is exactly a bf16 value; 1 | KURBM_V_BINARY promises that every element is 0.0 or 1.0, and the input is then staged as
 * the k-permuted BYTE plane in which the steps, the Gibbs runs and the score keep their 0/1 data and samples (one byte per
 * element, any non-zero element read as one) and multiplied by the same kernel instantiation as their half steps -- the only
 * way to call that kernel on its own.  With KURBM_X3_BYTES = 0 it is staged as one bf16 piece, as it is there.  The workspace is
 * kurbm_x3_workspace_bytes(rows, ..., in_pieces) for every format; all arguments are checked before anything is enqueued.
 * Exactness (tests/test_gpu_lattice.py holds every format to it bit for bit): where all operand values are multiples of
 * power-of-two quanta q_in and q_w, the bias of q_in * q_w, and sum_k |in_k| |w_k| + |bias| <= 2^22 q_in q_w for every output --
 * and, with in_pieces = 3, the three piece pairs that are left out vanish -- the pre-activation is the exact real-number result. */
int kurbm_half_step_x3(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, int dir,
                       const float* in, int in_pieces, int rows, int ld_in, int act, int noise,
                       const kurbm_rng* rng, float* out_sample, float* out_prob, float* out_u, int ld_out,
                       void* workspace, size_t workspace_bytes, kurbm_stream_t stream);

/* ---- data parallel: the exchange step ------------------------------------
 *
 * The reference has no multi-device path.  Each GPU runs the chain on its rows of the batch (rbm.py:119-124: rows
 * never interact) and the updates are SUMS over the batch (rbm.py:125-134), so ONE sum all-reduce of the packed
 * [dW | db_h | db_v] buffer reproduces the single-GPU update up to the order of the fp32 additions.  The collective
 * is RCCL's ncclAllReduce over xGMI, called from inside this library (bound at run time: librccl.so.1, or the file
 * KURBM_RCCL_LIB names); the host language only carries the 128-byte unique id from rank 0 to the other ranks.
 * One process per GPU: kurbm_comm_unique_id on rank 0, kurbm_comm_init_rank everywhere (collective: returns when all
 * ranks have joined).  One process driving several GPUs: kurbm_comm_init_all (ncclCommInitAll), `out` an array of ndev.
 */
#define KURBM_UNIQUE_ID_BYTES 128
int kurbm_comm_unique_id(void* id, size_t id_bytes);                                    /* ncclGetUniqueId  */
int kurbm_comm_init_rank(int device, int nranks, int rank, const void* id, size_t id_bytes,
                         kurbm_comm** out);                                             /* ncclCommInitRank */
int kurbm_comm_init_all(int ndev, const int* devs, kurbm_comm** out);                   /* ncclCommInitAll  */
int kurbm_comm_count(const kurbm_comm* comm);   /* ranks as RCCL reports them (ncclCommCount); < 0 = error */
int kurbm_comm_rank(const kurbm_comm* comm);    /* ncclCommUserRank; < 0 = error */
void kurbm_comm_destroy(kurbm_comm* comm);
/* In-place sum over all ranks of buf[0 .. n) (device fp32), ordered on `stream`. */
int kurbm_allreduce_sum_f32(kurbm_comm* comm, float* buf, size_t n, kurbm_stream_t stream);

/*
 * The data-parallel x3 step in ONE call: this rank's chain on its `rows` rows (opts->row0 = their global index), the
 * statistics GEMM in n_chunks row ranges of dW, each range's packed sums all-reduced on the library's comm stream
 * while the next range is still being computed on `stream` (db_h, db_v travel with the last range), then -- with
 * opts->apply = 1 -- W, b_h, b_v += lr * (summed delta) and the weight-piece mirror rewritten, in one launch, once the
 * last all-reduce has landed.  opts->delta_out (packed, required) holds the SUMMED statistics afterwards.  rows = 0
 * is legal (a rank that owns no rows of a remainder batch contributes zeros; v_batch is not read).  n_chunks <= 0:
 * ONE range, all-reduced on `stream` itself, whatever the size of the exchange (on MI355X / ROCm 7 the hand-off between two
 * streams costs more than a 3.2 MB all-reduce can hide, and the several-range schedule has not run at a world size above 1
 * yet) unless the context knob KURBM_DP_CHUNKS names a count -- DESIGN.md section 5.  Several ranges are an OPT-IN
 * (n_chunks > 1 or KURBM_DP_CHUNKS > 1): each one is then APPLIED (its rows of W, its part of the mirror) on the comm stream
 * as soon as its all-reduce has landed, under the statistics GEMM of the next; a HIP failure in that loop still joins the
 * comm stream back to `stream` before it is reported.  Every rank must pass the same n_chunks.  All work is ordered on
 * `stream` from the caller's point of view.
 * Every argument is checked before the first collective is enqueued, so a refused call has not joined an all-reduce
 * (the checks depend on arguments all ranks share; `rows` may differ).
 */
int kurbm_cd_step_x3_dp(kurbm_ctx* ctx, kurbm_comm* comm, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                        const float* v_batch, int v_pieces, int rows, int ldv, const kurbm_cd_opts* opts, int n_chunks,
                        void* workspace, size_t workspace_bytes, kurbm_stream_t stream);
/* The same step on the rounded-bf16 path (BASELINE.json config 5: 4096 x 4096, 67 MB of packed sums per step). */
int kurbm_cd_step_bf16_dp(kurbm_ctx* ctx, kurbm_comm* comm, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                          const float* v_batch, int rows, int ldv, const kurbm_cd_opts* opts, int n_chunks, void* workspace,
                          size_t workspace_bytes, kurbm_stream_t stream);

/* ---- small RBMs: one launch per step -----------------------------------------------------------------------------
 * The whole fused CD-1 update (rbm.py:120-134) of a SMALL problem -- the reference example's own 784 -> 128 at batch 128,
 * BASELINE.json configs[0] -- in ONE grid-resident launch (phases separated by device-scope barriers; csrc/kurbm_small.hip):
 * at these sizes the five launches of kurbm_cd_step are five launch latencies for a few microseconds of arithmetic.  Same
 * arguments, workspace (kurbm_workspace_bytes) and Philox counters as kurbm_cd_step; CD-1 from the data only (opts->k = 1,
 * no v_chain), applied in place (opts->apply = 1, no delta_out; `which` honoured).  Results agree with kurbm_cd_step to fp32
 * rounding (another summation order), not bit for bit.  The grid must be resident (at most one workgroup per CU, an otherwise
 * idle device); a barrier that times out sets bit 2 of kurbm_ctx_status and the update is skipped.  Where the context's probe
 * found the dispatcher dealing consecutive workgroups to consecutive XCDs (MI355X in SPX mode), phases 1-3 of a 16-row band of
 * the batch run inside ONE XCD -- the workgroups that find themselves on it -- and hand their planes over through its L2
 * (KURBM_SMALL_LOCAL, default 1; the launch is then always the whole device).  kurbm_cd_epoch_small: every batch of an epoch
 * in one call (returns the number of steps). */
int kurbm_cd_step_small(kurbm_ctx* ctx, const kurbm_params* p, const float* v_batch, int rows, int ldv,
                        const kurbm_cd_opts* opts, int which, void* workspace, size_t workspace_bytes, kurbm_stream_t stream);
int kurbm_cd_epoch_small(kurbm_ctx* ctx, const kurbm_params* p, const float* V, int n_rows, int ldv, int batch_size,
                         const kurbm_cd_opts* opts, void* workspace, size_t workspace_bytes, kurbm_stream_t stream);
/* ... and the per-step score of fit(verbose = 1), rbm.py:225-233, the same way: *score = mean |F(v) - F(v')| over the batch,
 * v' a fresh one-step reconstruction (opts->chain, sites 0 and 1, opts->seed / row0 / step / mode), in ONE launch with nothing
 * returned to the host; F (nullable, device [2 * rows]) receives F(v) then F(v').  At most 512 rows.  Workspace as for
 * kurbm_cd_step (kurbm_workspace_bytes).  Replaces the reference's four graph executions of its score (two free energies,
 * two sampling half steps). */
int kurbm_score_small(kurbm_ctx* ctx, const kurbm_params* p, const float* v_batch, int rows, int ldv, const kurbm_cd_opts* opts,
                      float* score, float* F, void* workspace, size_t workspace_bytes, kurbm_stream_t stream);
/* `score` is 8-byte aligned and receives TWO floats in one system-scope store: the score, then 1.0f -- so it may be pinned host
 * memory that the caller polls for the second word instead of synchronising with the device.  kurbm_cd_epoch_small_scored is
 * the batch loop of fit(verbose = 1) as one call: the update of every batch followed by its score (opts->step counts up for
 * both; the score draws from chain `score_chain`), scores[2 i], scores[2 i + 1] = the score of step i and its 1.0f.  Returns the
 * number of steps. */
int kurbm_cd_epoch_small_scored(kurbm_ctx* ctx, const kurbm_params* p, const float* V, int n_rows, int ldv, int batch_size,
                                const kurbm_cd_opts* opts, int score_chain, float* scores, void* workspace, size_t workspace_bytes,
                                kurbm_stream_t stream);

/* ---- data parallel, plan B: the exchange through peer pointers, no collective library ----------------------------
 *
 * A two-shot all-reduce over hipIpc-mapped buffers, its second shot fused into the launch that applies the update
 * (keras_unsupervised_amd/csrc/kurbm_peer.hip has the protocol).  Every rank: kurbm_peer_create (allocates and owns the
 * rank's exchange buffer for an n_vis x n_hid RBM), kurbm_peer_handle (its hipIpc handle, kurbm_peer_handle_bytes() bytes --
 * the host language carries the handles between the ranks, as it carries RCCL's unique id), kurbm_peer_connect with ALL
 * ranks' handles in rank order (maps the peers' buffers).  Then kurbm_cd_step_x3_peer in lock step on all ranks: the same
 * step as kurbm_cd_step_x3_dp with opts->apply = 1 (opts->delta_out is ignored: the sums live in the exchange buffers), sums
 * added in rank order, so every replica ends with identical bits.  n_hid % 4 == 0; at most 8 ranks.  A rank that fails an
 * argument check returns before it has published anything.  Every device-side wait is bounded (environment
 * KURBM_PEER_TIMEOUT_MS, default 10 000): a peer that never arrives sets bit 1 of kurbm_ctx_status and the update is skipped.
 * kurbm_peer_allreduce_sum_f32: the plain in-place sum of n <= n_vis n_hid + n_hid + n_vis floats (16-byte aligned), same protocol.
 * RCCL (kurbm_comm_*) stays the default exchange; this one also runs between PROCESSES THAT SHARE ONE GPU, which RCCL refuses.
 */
typedef struct kurbm_peer kurbm_peer;
size_t kurbm_peer_handle_bytes(void);
int kurbm_peer_create(int device, int nranks, int rank, int n_vis, int n_hid, kurbm_peer** out);
int kurbm_peer_handle(kurbm_peer* peer, void* handle, size_t handle_bytes);
int kurbm_peer_connect(kurbm_peer* peer, const void* handles, size_t bytes);
int kurbm_peer_ranks(const kurbm_peer* peer);
int kurbm_peer_allreduce_sum_f32(kurbm_ctx* ctx, kurbm_peer* peer, float* buf, size_t n, kurbm_stream_t stream);
int kurbm_cd_step_x3_peer(kurbm_ctx* ctx, kurbm_peer* peer, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                          const float* v_batch, int v_pieces, int rows, int ldv, const kurbm_cd_opts* opts, void* workspace,
                          size_t workspace_bytes, kurbm_stream_t stream);
void kurbm_peer_destroy(kurbm_peer* peer);

/* ---- momentum and L2 weight decay, fused into the launch that applies the update (extension) ----------------------
 *
 * The reference's rule is the bare theta += lr * sum_batch(pos - neg) (rbm.py:125-134).  The *_mom entry points apply the same
 * packed sums g (v_pos^T h_pos - v_neg^T h_neg and the bias column sums: bit for bit what opts->delta_out receives from the plain
 * step with the same counters) through a velocity, all in fp32:
 *     W   : vel <- momentum * vel + lr * (g - weight_decay * W) ;  W   <- W   + vel
 *     b_h : vel <- momentum * vel + lr * g                      ;  b_h <- b_h + vel      (no decay on biases; b_v likewise)
 * lr multiplies batch SUMS, so weight_decay is on the scale of those sums, not of a per-row mean (a mean-gradient recipe's
 * lambda times the batch size); the library does not rescale by the row count -- under data parallelism the apply sees only
 * the sum.  `vel` is caller-owned device memory in the layout of delta_out, packed [n_vis*n_hid | n_hid | n_vis] fp32 with no row
 * padding, 16-byte aligned, zeroed by the caller before the first step.  `which` masks as in kurbm_cd_step: a variable it does not
 * select has neither its parameters nor its velocity read or written.  The padding columns of W are left as they are.
 * The velocity travels inside the launch that already reduces the slabs and rewrites the weights (and, on the x3 / bf16 paths,
 * their bf16 pieces, which are made from the NEW weights): one more 16-byte load and store per weight group, no extra launch.
 * Every *_mom entry point takes the arguments of its plain twin plus `mom`, requires opts->apply = 1 and honours
 * opts->delta_out where the twin does (the same launch emits g).  KURBM_ERR_ARG, before anything is enqueued: mom or mom->vel null,
 * vel misaligned, momentum outside [0, 1), weight_decay < 0.  n_hid % 4 != 0 (velocity rows not 16-byte aligned) is served by the
 * two-launch form: update, then the mirror refresh.  The plain entry points are unchanged: they launch the kernels without any of this.
 */
typedef struct {
    float momentum;      /* mu in [0, 1) */
    float weight_decay;  /* lambda >= 0, on the scale of the batch sums */
    float* vel;          /* packed [n_vis*n_hid | n_hid | n_vis], 16-byte aligned */
} kurbm_momentum;

/* kurbm_cd_step / kurbm_cd_step_x3 / kurbm_cd_step_bf16 with the update applied through the velocity. */
int kurbm_cd_step_mom(kurbm_ctx* ctx, const kurbm_params* p, const float* v_batch, int rows, int ldv,
                      const kurbm_cd_opts* opts, int which, void* workspace, size_t workspace_bytes,
                      kurbm_stream_t stream, const kurbm_momentum* mom);
int kurbm_cd_step_x3_mom(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v_batch,
                         int v_pieces, int rows, int ldv, const kurbm_cd_opts* opts, int which, void* workspace,
                         size_t workspace_bytes, kurbm_stream_t stream, const kurbm_momentum* mom);
int kurbm_cd_step_bf16_mom(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v_batch,
                           int rows, int ldv, const kurbm_cd_opts* opts, int which, void* workspace, size_t workspace_bytes,
                           kurbm_stream_t stream, const kurbm_momentum* mom);
/* kurbm_cd_epoch / kurbm_cd_epoch_x3 likewise: one momentum and one weight_decay for every step of the call (a schedule over
 * epochs is the caller's: one call per epoch).  Returns the number of steps. */
int kurbm_cd_epoch_mom(kurbm_ctx* ctx, const kurbm_params* p, const float* V, int n_rows, int ldv, int batch_size,
                       const kurbm_cd_opts* opts, void* workspace, size_t workspace_bytes, kurbm_stream_t stream,
                       const kurbm_momentum* mom);
int kurbm_cd_epoch_x3_mom(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* V,
                          int v_pieces, int n_rows, int ldv, int batch_size, const kurbm_cd_opts* opts, void* workspace,
                          size_t workspace_bytes, kurbm_stream_t stream, const kurbm_momentum* mom);
/* kurbm_apply_delta / kurbm_x3_apply_delta likewise: the apply after a data-parallel exchange, g = the summed packed delta.  The
 * summed delta is the same on every rank, so the replicas' velocities stay identical. */
int kurbm_apply_delta_mom(kurbm_ctx* ctx, const kurbm_params* p, const float* delta, float lr, int which,
                          kurbm_stream_t stream, const kurbm_momentum* mom);
int kurbm_x3_apply_delta_mom(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* delta,
                             float lr, int which, kurbm_stream_t stream, const kurbm_momentum* mom);

/* *flag (device int, zeroed by the caller) |= 1 if some element of x [rows][ld] is not exactly representable in bf16,
 * |= 2 if some element is neither 0.0 nor 1.0.  0: v_pieces = 1 | KURBM_V_BINARY; 2: v_pieces = 1; else 3. */
int kurbm_bf16_exact(kurbm_ctx* ctx, const float* x, int rows, int cols, int ld, int* flag,
                     kurbm_stream_t stream);

/*
 * Annealed importance sampling (Salakhutdinov & Murray 2008) of log Z for a Bernoulli-Bernoulli RBM.  An extension: the
 * reference has no likelihood estimate at all (its score, rbm.py:225-233, is a reconstruction heuristic).
 * With b_A = base_bias (the visible bias of the base-rate model W = 0) and a(v) = v.W + b_h the intermediate distributions are
 *     p*_beta(v) = exp((1 - beta) b_A.v + beta b_v.v) prod_j (1 + exp(beta a_j(v))),
 * so log Z_0 = n_hid ln 2 + sum_i softplus(b_A,i) and p*_1 = exp(-F(v)).  Chain c (global index chain0 + c) runs
 *     v_0 = [u < sigmoid(b_A)]
 *     k = 1 .. n_betas - 1:   Delta_k = (beta_k - beta_{k-1}) (b_v - b_A).v_{k-1} + sum_j [softplus(beta_k a_j) - softplus(beta_{k-1} a_j)]
 *                             h = [u < sigmoid(beta_k a)],   v_k = [u < sigmoid((1 - beta_k) b_A + beta_k (h.W^T + b_v))]
 *     logw[c] = sum_k Delta_k                       (double; log Z ~ log Z_0 + log mean_c exp(logw[c]) is the caller's)
 * Draws follow the Philox contract above with row = chain0 + c (any value, not only multiples of 4), col = unit, step = k and
 * the three sampling sites below (v_0: step 0).  One temperature is two fp32-MFMA GEMM launches -- the half steps with beta in
 * the epilogue; W is never scaled -- and one small launch that adds Delta_k into logw; the softplus difference is evaluated as
 * log1p(sigmoid(beta_{k-1} a) expm1((beta_k - beta_{k-1}) a)), which does not cancel at the 1e-4 spacing of a long run.  The
 * whole run is queued without a host synchronisation, and is bit-reproducible for (seed, betas, chain0): a chain's numbers do
 * not depend on how many other chains share the call.
 * betas is a HOST array (read before the call returns): betas[0] = 0, betas[n_betas - 1] = 1, strictly increasing.
 * v_final (nullable): the chains' last visibles.  KURBM_ERR_ARG for a bad schedule, a leading dimension below the column count
 * or a null / misaligned buffer, KURBM_ERR_WORKSPACE for ws_bytes < kurbm_ais_workspace_bytes: nothing is written then.
 */
#define KURBM_STREAM_AIS_INIT 0x200u
#define KURBM_STREAM_AIS_H    0x201u
#define KURBM_STREAM_AIS_V    0x202u
size_t kurbm_ais_workspace_bytes(kurbm_ctx* ctx, int n_chains, int n_vis, int n_hid);
int kurbm_ais_run(kurbm_ctx* ctx, const kurbm_params* p, const float* base_bias, const double* betas, int n_betas,
                  int n_chains, uint64_t chain0, uint64_t seed, double* logw, float* v_final, int ldv,
                  void* ws, size_t ws_bytes, kurbm_stream_t stream);
/*
 * Test hook: temperature k of such a run, teacher-forced -- the same three launches on the caller's v_in [n_chains][ldv].
 * dlogw[c] = Delta_k; h [n_chains][ldh] and v_out [n_chains][ldvo] the samples (v_out is drawn from the call's own h).
 * Nullable test planes: prob_h, u_h (ldh) and prob_v, u_v (ldvo), the probabilities and the uniforms they were compared with.
 * 0 <= beta_prev < beta <= 1, k >= 1.
 */
int kurbm_ais_step(kurbm_ctx* ctx, const kurbm_params* p, const float* base_bias, double beta_prev, double beta, int k,
                   const float* v_in, int ldv, int n_chains, uint64_t chain0, uint64_t seed, float* dlogw,
                   float* h, int ldh, float* v_out, int ldvo, float* prob_h, float* u_h, float* prob_v, float* u_v,
                   void* ws, size_t ws_bytes, kurbm_stream_t stream);

/*
 * Gibbs runs: samples from a trained RBM (fantasy particles, conditional completions), both visible modes.  An extension: the
 * reference offers one half step per call (transform_func / inv_transform_func, rbm.py:46-54, :58-67) and no clamping.
 * From v_0 = v_init, sweep t = 1 .. T, T = burn_in + (n_keep - 1) * thin:
 *     h_t = draw(p(h | v_{t-1})),   v_t = draw(p(v | h_t)),   then v_t[:, c] = v_init[:, c] for every clamped unit c.
 * The sites are those of the half steps for `mode`: Bernoulli visibles h = [u < sigmoid(v.W + b_h)], v = [u < sigmoid(h.W^T + b_v)];
 * Gaussian visibles h = [u < relu(v.W + b_h)], v = (h.W^T + b_v) + z.  Draws follow the Philox contract above with
 * row = chain0 + chain, col = unit, step = t and the two stream ids below; chain0 % 4 == 0.
 * Kept sample j (0 <= j < n_keep) is v_{burn_in + j * thin}, written to v_out + j * keep_stride as fp32 [n_chains][ldo];
 * prob_out (nullable, same layout) receives the activated value it was drawn from -- the probability of Bernoulli visibles, the
 * mean of Gaussian ones.  Clamped columns hold v_init's value in both.  burn_in, thin, n_keep >= 1.
 * v_pieces describes v_init as for kurbm_cd_step_x3 (1 | KURBM_V_BINARY: every element 0.0 or 1.0; 1: exactly bf16; 3: any fp32).
 * clamp (nullable) is a DEVICE array of n_vis bytes, non-zero = clamped; it is read by the run's launches, not by the host.
 * One sweep is the two x3 half-step launches (bf16 matrix cores, products exact, fp32 accumulation); the states never leave their
 * operand format -- byte planes for 0/1 states, three bf16 pieces for Gaussian visibles -- and only kept sweeps write fp32 planes.
 * A mask adds one small launch per sweep (and one per run that lays the mask out in the planes' order).  Nothing is read back,
 * nothing synchronises, the library allocates nothing.  The same call twice gives identical bits.  A chain's numbers are NOT
 * promised to be independent of n_chains: the planner picks the tile shape by the row count, and with it the order of the fp32
 * additions (the uniforms of a chain are the same whatever the count).
 * Padding columns [n_vis, ld) of v_init are not read into a result; those of v_out / prob_out are not written.
 * KURBM_ERR_ARG / KURBM_ERR_WORKSPACE, before anything is enqueued: a null or misaligned buffer, ld < n_vis or ld % 4 != 0,
 * keep_stride < n_chains * ldo (or not a multiple of 4) when n_keep > 1, a count below 1, chain0 & 3, an unknown v_pieces or mode,
 * mirror_bytes < kurbm_x3_mirror_bytes, ws_bytes < kurbm_gibbs_workspace_bytes (0 for a bad shape).  The mirror is the x3 mirror.
 */
#define KURBM_STREAM_GIBBS_H 0x210u
#define KURBM_STREAM_GIBBS_V 0x211u   /* Gaussian visibles: normals from this plane and | 0x80000000, as everywhere */
size_t kurbm_gibbs_workspace_bytes(kurbm_ctx* ctx, int n_chains, int n_vis, int n_hid, int v_pieces, int mode);
int kurbm_gibbs_run(kurbm_ctx* ctx, const kurbm_params* p, void* mirror, size_t mirror_bytes, const float* v_init, int v_pieces,
                    int ldv, int n_chains, uint64_t chain0, uint64_t seed, int mode, int burn_in, int thin, int n_keep,
                    const uint8_t* clamp, float* v_out, float* prob_out, int ldo, size_t keep_stride, void* ws, size_t ws_bytes,
                    kurbm_stream_t stream);

/*
 * Softmax label units: joint training on [pixels | one-hot label], exact class posteriors.  An extension: the reference's only road
 * from an RBM to a class is a separate softmax head on sampled features (examples/rbm/rbm_softmax_mnist.py).
 * A label RBM has n_vis = n_pix + C visible units, 2 <= C = n_labels <= 64; the LAST C columns are the label block -- rows
 * n_pix .. n_vis-1 of W, entries n_pix .. n_vis-1 of b_v.  Bernoulli visibles only.  Exactly one unit of the block is on.
 *   Label site, given the hidden states h of a row:
 *     x_c = b_v[n_pix + c] + sum_j h_j W[n_pix + c][j];   p = softmax(x) in fp32: subtract the max, exp, sum in class order, divide;
 *     u = u(row, col = n_pix) under the Philox contract above -- ONE uniform per row, stream id and step those of the h -> v site
 *     the block belongs to (chain*64 + 2t-1 inside a CD step);  the drawn class is the first c with u < p_0 + ... + p_c (running
 *     fp32 sum in class order), else C-1;  the block becomes that one-hot vector.  A row's p and draw do not depend on how many
 *     rows share the launch; every reduction order is fixed and nothing is atomic.
 *   Class logits, for pixels v (any real values), a = v.W[:n_pix] + b_h:
 *     logit_c = b_v[n_pix + c] + sum_j softplus(a_j + W[n_pix + c][j])      (the overflow-free softplus of kurbm_free_energy)
 *     p(y = c | v) = softmax_c(logit);   F(v, y = c) = -v.b_v[:n_pix] - logit_c.
 *   CD step with labels = kurbm_cd_step on the n_vis-wide batch, except that after EVERY h -> v half step the block of that v_t is
 *     rewritten by the label site (so a persistent chain keeps one-hot blocks), and for the last v_t the label columns of the
 *     visible-bias sums become sum_rows(v_batch - v_neg) over the new block; h_neg, the statistics and the apply see that v_neg.
 *     The positive phase and the v -> h half steps need nothing: a one-hot block is 0/1 columns.
 * The x3 / bf16 / one-launch TRAINING paths have no label site: a label RBM trains on the fp32 five-launch path.  The Gibbs and AIS
 * runs have one: "free label blocks" below.
 * KURBM_ERR_ARG, before anything is enqueued, for n_labels outside [2, 64] or >= n_vis, a mode other than Bernoulli, and whatever
 * the plain twin refuses; KURBM_ERR_WORKSPACE for a short workspace.
 *
 * kurbm_label_sample: the label site alone (test hook; the host's inv_transform).  h [rows][ldh] fp32 (read as real values); the
 * label columns of v [rows][ldv] are written as fp32 0/1 -- its pixel and padding columns are neither read nor written; prob
 * (nullable) [rows][ldp] receives p, out_u (nullable) [rows] the uniforms.  rng->row0 % 4 == 0.
 */
int kurbm_label_sample(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* h, int rows, int ldh,
                       const kurbm_rng* rng, float* v, int ldv, float* prob, int ldp, float* out_u, kurbm_stream_t stream);
/* kurbm_cd_step / kurbm_cd_step_mom (mom null / not null) and kurbm_cd_epoch / kurbm_cd_epoch_mom with the label site: the fp32
 * launches of the plain step plus one small launch per h -> v half step.  k, v_chain, apply, delta_out, which, row0, chain and
 * mom are honoured exactly as there; the workspace is that of kurbm_workspace_bytes (with its ldv addition), nothing more. */
int kurbm_cd_step_labels(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* v_batch, int rows, int ldv,
                         const kurbm_cd_opts* opts, int which, void* workspace, size_t workspace_bytes, kurbm_stream_t stream,
                         const kurbm_momentum* mom /* nullable */);
int kurbm_cd_epoch_labels(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* V, int n_rows, int ldv, int batch_size,
                          const kurbm_cd_opts* opts, void* workspace, size_t workspace_bytes, kurbm_stream_t stream,
                          const kurbm_momentum* mom /* nullable */);
/* Class logits [rows][ldl] and, nullable, their softmax prob [rows][ldl] (same leading dimension) in two launches: the linear
 * v -> h half step on the pixel rows of W (they are its top rows: nothing is copied) into the workspace, then one launch that reads
 * that plane once with all C classes in registers.  v needs only n_pix valid columns (ldv >= n_pix); a label block behind them is
 * ignored.  Workspace: kurbm_class_workspace_bytes (0 for a bad shape). */
size_t kurbm_class_workspace_bytes(kurbm_ctx* ctx, int rows, int n_vis, int n_hid);
int kurbm_class_logits(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* v, int rows, int ldv, float* logits,
                       int ldl, float* prob, void* workspace, size_t workspace_bytes, kurbm_stream_t stream);

/*
 * Discriminative and hybrid training of a label RBM (Larochelle & Bengio 2008, "Classification using discriminative restricted
 * Boltzmann machines").  The posterior above is differentiable in closed form; its gradient is exact and needs no Gibbs chain and no
 * random number.  With n_vis = n_pix + C, U = W[n_pix:] (C x n_hid), d = b_v[n_pix:], a = v_pix.W[:n_pix] + b_h, o_cj = a_j + U_cj,
 * logit_c = d_c + sum_j softplus(o_cj), p = softmax(logit), t the one-hot block of the row and y the class that is on (the first
 * unit above 1/2; the callers have checked the block), per row:
 *     nll    = logsumexp_c(logit) - logit_y            (from the logits, never as -log p_y: finite where p_y has underflowed)
 *     q_c    = t_c - p_c
 *     S_y[j] = sigmoid(o_yj)      H_bar[j] = sum_c p_c sigmoid(o_cj)      g_j = S_y[j] - H_bar[j] = sum_c q_c sigmoid(o_cj)
 * and as batch SUMS, like every update rule of this library, the gradient of sum_rows log p(y | v):
 *     dW[:n_pix] = v_pix^T.S_y - v_pix^T.H_bar       db_h = sum_rows g
 *     dU[c][j]   = sum_rows q_c sigmoid(o_cj)        dd_c = sum_rows q_c        db_v[:n_pix] = 0
 * The update is params += lr * delta through kurbm_apply_delta (kurbm_apply_delta_mom with `mom`).  The hybrid objective
 * log p(y | v) + gen_weight * log p(v, y) makes ONE update per batch, delta = delta_disc + gen_weight * delta_gen (each product
 * rounded to fp32, then one fp32 addition), delta_gen being the packed delta kurbm_cd_step_labels emits (apply = 0) on the same
 * batch at the same weights with the step's own RNG coordinates: both gradients are taken at the same parameters and the velocity
 * moves once.
 * Launches of one gradient: the linear v -> h half step on the pixel rows of W and the class-logit launch (those of
 * kurbm_class_logits), k_class_grad (the plane g, nll, row-tile partials of dU, dd and db_h; S_y and H_bar only for the test hook),
 * the statistics GEMM of the pixel rows as ONE segment, v_pix^T.g with g = fl(S_y - H_bar) -- half the work of the two-segment
 * form -- and the reduction of its slabs, and one launch that sums the partials in tile order into the packed delta.  Nothing is
 * atomic and every sum runs in one fixed order: a call is a deterministic function of its inputs, and a row's S_y, H_bar and nll do
 * not depend on how many rows share the call.
 *
 * kurbm_disc_workspace_bytes: the scratch of all three calls for batches of <= rows (0 for a bad shape).  A hybrid step
 * (gen_weight > 0) on a batch with ldv > round_up(n_vis, 4) needs the addition kurbm_workspace_bytes states, for the same reason.
 * kurbm_class_grad (test hook): the planes S_y, H_bar [rows][ldh], nll [rows] (all three nullable) and the packed delta_out
 *   [dW | db_h | db_v] (required) of v_batch [rows][ldv], whose last n_labels columns are the one-hot block.  Nothing is applied.
 * kurbm_disc_step: one update.  gen_weight == 0: discriminative; > 0: hybrid, the generative chain running through the label-step
 *   machinery with opts->k, v_chain, seed, step, row0, chain.  opts->lr is the learning rate; opts->mode must be Bernoulli;
 *   opts->apply, delta_out and v_planes are not read.  nll_mean (nullable, device float) receives the batch's mean nll BEFORE the update.
 * kurbm_disc_epoch: contiguous batches of V [n_rows][ldv], remainder last, opts->step advancing by one per batch, no host round
 *   trip; nll_means (nullable, device [number of batches]) receives each batch's mean.  Returns the number of steps (>= 0).
 * KURBM_ERR_ARG / KURBM_ERR_WORKSPACE, before anything is enqueued and with nothing written: n_labels outside [2, 64] or >= n_vis,
 * a negative or non-finite gen_weight, a null or misaligned buffer, ld % 4 != 0 or below the column count, a mode other than
 * Bernoulli, a bad momentum block, ws_bytes below the query, and (hybrid) whatever kurbm_cd_step_labels refuses.
 */
size_t kurbm_disc_workspace_bytes(kurbm_ctx* ctx, int rows, int n_vis, int n_hid, int n_labels);
int kurbm_class_grad(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* v_batch, int rows, int ldv, float* S_y,
                     float* H_bar, int ldh, float* nll, float* delta_out, void* ws, size_t ws_bytes, kurbm_stream_t stream);
int kurbm_disc_step(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* v_batch, int rows, int ldv,
                    const kurbm_cd_opts* opts, float gen_weight, float* nll_mean /* nullable */, void* ws, size_t ws_bytes,
                    kurbm_stream_t stream, const kurbm_momentum* mom /* nullable */);
int kurbm_disc_epoch(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* V, int n_rows, int ldv, int batch_size,
                     const kurbm_cd_opts* opts, float gen_weight, float* nll_means /* nullable */, void* ws, size_t ws_bytes,
                     kurbm_stream_t stream, const kurbm_momentum* mom /* nullable */);

/*
 * Fine-tuning a DBN: backpropagation of sum_rows log p(y | v) through its layers (Hinton & Salakhutdinov 2006; Larochelle & Bengio
 * 2008, section 6).  The stack is layers l = 1 .. L-1, plain RBMs (W_l [n_{l-1}, n_l], b_h,l), under a top label RBM with
 * n_pix = n_{L-1}, C classes and (W, b_h, b_v).  Batch SUMS, like every update rule of this library.
 *   Forward, the mean-field path of DBN.predict_proba:  x_0 = v;  x_l = act_l(x_{l-1}.W_l + b_h,l) -- the prob-only v -> h half step,
 *     sigmoid (Bernoulli mode) or relu (Gaussian mode), no draw;  the top layer sees [x_{L-1} | one-hot(y)].
 *   Top layer: g, nll and the packed delta [dW | db_h | db_v] of "discriminative and hybrid training" above, and
 *     e_{L-1} = g . W[:n_pix]^T                          (rows x n_pix, NO bias term)
 *   Layer l, going down from L-1, given e_l = dL/dx_l:
 *     delta_l = e_l * act_l'(x_l)        sigmoid: x_l (1 - x_l);  relu: [x_l > 0];  linear (tests): 1
 *     dW_l = x_{l-1}^T . delta_l         db_h,l = sum_rows delta_l         db_v,l = 0
 *     e_{l-1} = delta_l . W_l^T          (no bias; not needed for l = 1)
 *   Update: every layer's delta is taken at the weights the step started from; the applies come after the last backward launch, each
 *     layer params += lr * delta through kurbm_apply_delta / kurbm_apply_delta_mom.
 * Launches of a layer: k_backprop_delta (delta in place over e, row-tile partials of db_h), k_backprop_reduce (the partials in tile
 * order, in double, rounded once, into db_h; zeros into db_v), the statistics GEMM x_{l-1}^T.delta as ONE segment with the reduction
 * of its slabs into dW, and, where e_in is wanted, the linear h -> v half step delta.W^T whose bias is the db_v block just zeroed:
 * the fp32-MFMA launches of the steps above, unchanged.  No allocation, no host synchronisation, no random number, nothing atomic,
 * every sum in one fixed order: a call is a deterministic function of its inputs, and a row's delta and e_in do not depend on how
 * many rows share the call.
 *
 * kurbm_backprop_workspace_bytes: the scratch of kurbm_backprop_layer on a layer of n_in x n_out units for batches of <= rows (0 for
 *   a bad shape).  kurbm_backprop_delta takes the query at n_in = 1.
 * kurbm_backprop_delta (test hook): the site alone.  e, x_out [rows][n_hid]; delta [rows][ldd] (it may equal e, with ldd == lde);
 *   db_h [n_hid].  Columns [n_hid, ld) of every plane are neither read into a result nor written.
 * kurbm_backprop_layer: p = the layer's parameters (b_h and b_v are not read, but the block is checked as everywhere), x_in [rows][ldin] its input (n_vis columns), x_out [rows][ldout]
 *   its output as the forward pass left it, e [rows][lde] dL/dx_out on entry and delta on return, delta_out the packed
 *   [dW | db_h | db_v = 0] (required), e_in (nullable) [rows][ldei] dL/dx_in.  delta_out does not depend on whether e_in is given.
 * kurbm_disc_backprop: the launches of kurbm_class_grad on v_batch [rows][ldv] (label block last), then e_in (nullable)
 *   [rows][ldei] = g.W[:n_pix]^T.  Nothing is applied.  delta_out and nll_mean (nullable, device float: the batch's mean nll) are bit
 *   for bit those of kurbm_class_grad / kurbm_disc_step on the same batch.  Workspace: kurbm_disc_workspace_bytes, nothing more (the
 *   product reads the plane g there, and its zero bias is db_v[:n_pix] of delta_out).
 * KURBM_ERR_ARG / KURBM_ERR_WORKSPACE, before anything is enqueued and with nothing written: a null or misaligned buffer, ld % 4 != 0
 * or below the column count, an act that is none of KURBM_ACT_*, rows <= 0, ws_bytes below the query, and for kurbm_disc_backprop
 * whatever kurbm_class_grad refuses.
 */
size_t kurbm_backprop_workspace_bytes(kurbm_ctx* ctx, int rows, int n_in, int n_out);
int kurbm_backprop_delta(kurbm_ctx* ctx, const float* e, int lde, const float* x_out, int ldx, int rows, int n_hid, int act,
                         float* delta, int ldd, float* db_h, void* ws, size_t ws_bytes, kurbm_stream_t stream);
int kurbm_backprop_layer(kurbm_ctx* ctx, const kurbm_params* p, int act, const float* x_in, int ldin, const float* x_out, int ldout,
                         float* e, int lde, int rows, float* delta_out, float* e_in /* nullable */, int ldei, void* ws,
                         size_t ws_bytes, kurbm_stream_t stream);
int kurbm_disc_backprop(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* v_batch, int rows, int ldv,
                        float* delta_out, float* e_in /* nullable */, int ldei, float* nll_mean /* nullable */, void* ws,
                        size_t ws_bytes, kurbm_stream_t stream);

/*
 * Free label blocks: the softmax site inside the Gibbs and AIS runs, so that a label RBM is the generative model it was trained as --
 * joint samples (v, y), a sampled class for given pixels, and log Z of p(v, y).  n_pix = n_vis - C; the block is the last C columns;
 * Bernoulli visibles only.  The label site is the one stated under "softmax label units".
 *
 * Gibbs sweep t with a free block (kurbm_gibbs_run_labels; everything else as kurbm_gibbs_run):
 *     h_t as there: the one-hot block of v_{t-1} is ordinary 0/1 columns.  The pixels of v_t as there.
 *     The block of v_t is then ONE draw of softmax(x), x_c = b_v[n_pix + c] + sum_j h_t,j W[n_pix + c][j]: subtract the max, exp, sum in
 *     class order, divide; the drawn class is the first c with u < p_0 + ... + p_c on a running fp32 sum, else C-1;
 *     u = u(chain0 + chain, col n_pix) at (KURBM_STREAM_GIBBS_V, step t): one uniform per row.
 *     After the block is drawn, clamped pixels are copied back as there.
 *     On a kept sweep the block of v_out is the one-hot vector and the block of prob_out is p.
 *   W is read as the fp32 master rows, not the mirror; h is read from the run's hidden plane (bytes or one bf16 piece: exactly 0 / 1),
 *   and the block is written into the current visible plane in its format.  One small launch per sweep, in front of the clamp launch.
 *   Every sum runs in a fixed order and nothing is atomic: the same call twice gives identical bits.
 *   `mode` must be KURBM_MODE_VISIBLE_BERNOULLI.  The label columns of `clamp` are NOT read: the block is free here, and a clamped
 *   block is kurbm_gibbs_run's business.  The workspace is that of kurbm_gibbs_workspace_bytes.
 *
 * AIS with a label block (kurbm_ais_run_labels; everything else as kurbm_ais_run), over v = [pixels | one-hot], a = v.W + b_h on
 * all n_vis columns:
 *     p*_beta(v) = exp((1 - beta) b_A.v + beta b_v.v) prod_j (1 + exp(beta a_j(v)))
 *     log Z_0 = n_hid ln 2 + sum_{i < n_pix} softplus(b_A,i) + logsumexp_c b_A[n_pix + c]
 *     start:  pixels [u < sigmoid(b_A)]; the class from softmax(b_A[n_pix:]) by the site's recipe, u = u(row, n_pix) at
 *             (KURBM_STREAM_AIS_INIT, 0)
 *     k:      Delta_k = dbeta (sum_{i < n_pix} (b_v - b_A)_i v_i + (b_v - b_A)[n_pix + y]) + sum_j [softplus(beta_k a_j) - softplus(beta_{k-1} a_j)]
 *             h and the pixels as there; the block is one draw of softmax(x),
 *             x_c = (1 - beta_k) b_A[n_pix + c] + beta_k (b_v[n_pix + c] + sum_j h_j W[n_pix + c][j]), u = u(row, n_pix) at (KURBM_STREAM_AIS_V, k).
 *   One temperature is the two GEMM launches of kurbm_ais_run -- the h -> v one on the n_pix pixel rows of W -- the label site on the
 *   fp32 hidden plane, and the accumulate launch.  The site's row partial needs one group row more than kurbm_ais_workspace_bytes
 *   holds at some shapes (n_pix = 33, C = 2): the size query is kurbm_ais_labels_workspace_bytes (0 for a bad shape).
 * kurbm_ais_step_labels: the test hook, teacher-forced like kurbm_ais_step; v_in [n_chains][ldv] carries a one-hot block (its class is
 *   the first unit above 1/2).  Additional nullable planes prob_y [n_chains][ldp] (the block's p) and u_y [n_chains].  The label
 *   columns of prob_v / u_v are not written.
 * KURBM_ERR_ARG, before anything is enqueued and with nothing written: n_labels outside [2, 64] or >= n_vis, a mode other than
 * Bernoulli, and whatever the plain twin refuses; KURBM_ERR_WORKSPACE for short buffers.
 */
int kurbm_gibbs_run_labels(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, void* mirror, size_t mirror_bytes, const float* v_init,
                           int v_pieces, int ldv, int n_chains, uint64_t chain0, uint64_t seed, int mode, int burn_in, int thin,
                           int n_keep, const uint8_t* clamp, float* v_out, float* prob_out, int ldo, size_t keep_stride, void* ws,
                           size_t ws_bytes, kurbm_stream_t stream);
size_t kurbm_ais_labels_workspace_bytes(kurbm_ctx* ctx, int n_chains, int n_vis, int n_hid, int n_labels);
int kurbm_ais_run_labels(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* base_bias, const double* betas, int n_betas,
                         int n_chains, uint64_t chain0, uint64_t seed, double* logw, float* v_final, int ldv, void* ws, size_t ws_bytes,
                         kurbm_stream_t stream);
int kurbm_ais_step_labels(kurbm_ctx* ctx, const kurbm_params* p, int n_labels, const float* base_bias, double beta_prev, double beta,
                          int k, const float* v_in, int ldv, int n_chains, uint64_t chain0, uint64_t seed, float* dlogw, float* h,
                          int ldh, float* v_out, int ldvo, float* prob_h, float* u_h, float* prob_v, float* u_v, float* prob_y, int ldp,
                          float* u_y, void* ws, size_t ws_bytes, kurbm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KURBM_H */
