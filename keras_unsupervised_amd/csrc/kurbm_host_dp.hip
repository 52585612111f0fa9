// kurbm_host_dp.hip -- the data-parallel CD steps of the C ABI (include/kurbm.h): the all-reduce of the packed sums through RCCL
// (kurbm_comm.hip) and through the peer exchange (kurbm_peer.hip), around the local step of kurbm_host_x3.hip.
#include <string>

#include "kurbm_host.h"

using namespace kurbm;

// Row ranges of dW in the data-parallel step.  The AUTOMATIC choice (n_chunks <= 0, knob KURBM_DP_CHUNKS unset) is ONE range,
// all-reduced on the caller's stream, whatever the size of the exchange: on MI355X / ROCm 7 a hand-off between two HIP streams
// costs 12-16 us per event wait and a statistics GEMM cut in two ~13 us (tools/dp_times.py) -- ~49 us before a second range's
// all-reduce can start, more than the half of a 3.2 MB exchange it could hide -- and the several-range schedule (range i
// all-reduced and applied on the comm stream under the statistics GEMM of range i + 1) has never run at a world size above 1
// (tests/test_two_gpus.py is skipped on every box this build has seen).  It stays in the tree as an OPT-IN: the caller's
// n_chunks > 1, or KURBM_DP_CHUNKS > 1 (every rank must pass the same value), e.g. 4 ranges of ~16 MiB for the 67 MB of a
// 4096 x 4096 RBM once tests/test_two_gpus.py has passed on a real node.
constexpr int AUTO_CHUNKS = 1;

static int cd_step_dp_any(kurbm_ctx* ctx, kurbm_comm* comm, int pieces, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                          const float* v_batch, int v_pieces, int rows, int ldv, const kurbm_cd_opts* opts, int n_chunks,
                          void* workspace, size_t workspace_bytes, kurbm_stream_t stream) {
    if (!ctx || !comm || !opts) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_params(p)) return e;
    if (!opts->delta_out || !aligned16(opts->delta_out)) return fail_msg(KURBM_ERR_ARG, "delta_out (the packed sums) is required, 16-byte aligned");
    if (comm->device != ctx->device) return fail_msg(KURBM_ERR_ARG, "communicator is on device %d, context on %d", comm->device, ctx->device);
    if (rows < 0) return fail_msg(KURBM_ERR_ARG, "rows must be >= 0");
    // everything cd_step_any would refuse is refused HERE, before the first collective is enqueued: a rank that returned
    // an error from inside the sequence would leave the other ranks waiting in ncclAllReduce
    if (int e = check_cd_args(ctx, pieces, v_pieces, p, mirror, mirror_bytes, v_batch, rows, ldv, opts, workspace, workspace_bytes, true)) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t nw = (size_t)p->n_vis * p->n_hid, ntot = nw + p->n_hid + p->n_vis;
    // row ranges of dW: boundaries on multiples of 128 (the statistics tile), the same on every rank
    if (n_chunks <= 0) n_chunks = knob(ctx, KN_DP_CHUNKS) > 0 ? knob(ctx, KN_DP_CHUNKS) : AUTO_CHUNKS;
    if (n_chunks > kurbm_comm::MAX_CHUNKS) n_chunks = kurbm_comm::MAX_CHUNKS;
    int bound[kurbm_comm::MAX_CHUNKS + 1];
    int nc = 0;
    bound[0] = 0;
    for (int c = 1; c < n_chunks; ++c) {
        const int b = (int)((long long)p->n_vis * c / n_chunks) / 128 * 128;
        if (b > bound[nc] && b < p->n_vis) bound[++nc] = b;
    }
    bound[++nc] = p->n_vis;
    kurbm_cd_opts o = *opts;
    o.apply = 0;
    // several ranges: each one is applied (W rows, the mirror's pieces of those rows) on the comm stream as soon as its
    // all-reduce has landed, under the statistics GEMM of the next; that needs 16-byte-aligned rows in the packed buffer
    const bool apply_ranges = opts->apply && nc > 1 && (p->n_hid & 3) == 0;
    if (rows == 0) HIP_TRY(hipMemsetAsync(o.delta_out, 0, ntot * sizeof(float), st));
    else if (nc > 1)
        if (int e = cd_step_any(ctx, pieces, v_pieces, p, mirror, mirror_bytes, v_batch, rows, ldv, &o, 7, workspace, workspace_bytes, stream, 8))
            return e;
    // Once the first collective of a several-range step is enqueued, this rank must finish the sequence as far as the other
    // ranks can see it: a failure inside the loop (a HIP error of a launch or an event call) still records ev_done on the comm
    // stream and makes the caller's stream wait for it before the error is returned -- the comm stream never stays ahead of
    // the caller's, and the collectives already enqueued complete against the peers' matching ones.  (Argument errors cannot
    // occur here: check_cd_args ran before anything was enqueued.)
    int err = KURBM_OK;
    bool on_comm = false;
    auto range = [&](int c) -> int {
        if (rows > 0) {
            const int e = (nc == 1)
                ? cd_step_any(ctx, pieces, v_pieces, p, mirror, mirror_bytes, v_batch, rows, ldv, &o, 7, workspace, workspace_bytes, stream)
                : cd_step_any(ctx, pieces, v_pieces, p, mirror, mirror_bytes, v_batch, rows, ldv, &o, 7, workspace, workspace_bytes, stream, 7,
                              bound[c], bound[c + 1]);
            if (e) return e;
        }
        const size_t lo = (size_t)bound[c] * p->n_hid, hi = (c + 1 == nc) ? ntot : (size_t)bound[c + 1] * p->n_hid;
        if (nc == 1)    // nothing to overlap with: the all-reduce stays on the caller's stream, no hand-off
            return comm_allreduce_sum(comm, o.delta_out + lo, hi - lo, st);
        // this range's sums are complete on `stream`: hand them to the comm stream
        HIP_TRY(hipEventRecord(comm->ev_ready[c], st));
        HIP_TRY(hipStreamWaitEvent(comm->stream, comm->ev_ready[c], 0));
        on_comm = true;
        if (int e = comm_allreduce_sum(comm, o.delta_out + lo, hi - lo, comm->stream)) return e;
        if (apply_ranges)
            return apply_delta_rows(ctx, p, mirror, mirror_bytes, pieces, o.delta_out, o.lr, 7, bound[c], bound[c + 1], c + 1 == nc, comm->stream);
        return KURBM_OK;
    };
    for (int c = 0; c < nc && !err; ++c) err = range(c);
    if (on_comm) {   // (also on the error path: see above)
        const std::string keep = kurbm_last_error();
        const hipError_t e1 = hipEventRecord(comm->ev_done, comm->stream);
        const hipError_t e2 = (e1 == hipSuccess) ? hipStreamWaitEvent(st, comm->ev_done, 0) : e1;
        if (err) fail_msg(err, "%s", keep.c_str());
        else if (e2 != hipSuccess) err = fail_msg(KURBM_ERR_HIP, "joining the comm stream: %s", hipGetErrorString(e2));
    }
    if (err) return err;
    if (opts->apply && !apply_ranges) {
        if (pieces == 3) return kurbm_x3_apply_delta(ctx, p, mirror, mirror_bytes, o.delta_out, o.lr, 7, stream);
        if ((p->n_hid & 3) == 0) return apply_delta_rows(ctx, p, mirror, mirror_bytes, pieces, o.delta_out, o.lr, 7, 0, p->n_vis, true, st);
        if (int e = kurbm_apply_delta(ctx, p, o.delta_out, o.lr, 7, stream)) return e;
        return mirror_refresh_any(ctx, pieces, p, mirror, mirror_bytes, stream);
    }
    return KURBM_OK;
}

extern "C" {

// The data-parallel x3 step on the PEER exchange (kurbm_peer.hip): chain -> statistics -> slab reduce into this rank's exported
// `delta` region -> shot 1 (every rank sums its band of all ranks' deltas, in rank order) -> ONE launch that reads every band
// from its owner's `sum` region and applies it (W, biases, both weight-piece mirrors).  Two launches beyond the local step's own.
int kurbm_cd_step_x3_peer(kurbm_ctx* ctx, kurbm_peer* peer, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                          const float* v_batch, int v_pieces, int rows, int ldv, const kurbm_cd_opts* opts, void* workspace,
                          size_t workspace_bytes, kurbm_stream_t stream) {
    if (!ctx || !peer || !opts) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (int e = check_params(p)) return e;
    if (int e = peer_geometry_ok(peer, ctx->device, p->n_vis, p->n_hid)) return e;
    if (!opts->apply) return fail_msg(KURBM_ERR_ARG, "kurbm_cd_step_x3_peer applies the summed update in place: apply = 1");
    if (rows < 0) return fail_msg(KURBM_ERR_ARG, "rows must be >= 0");
    // everything the step would refuse is refused HERE, before this rank publishes anything a peer waits for
    if (int e = check_cd_args(ctx, 3, v_pieces, p, mirror, mirror_bytes, v_batch, rows, ldv, opts, workspace, workspace_bytes, true)) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t nw = (size_t)p->n_vis * p->n_hid, ntot = nw + p->n_hid + p->n_vis;
    kurbm_cd_opts o = *opts;
    o.apply = 0;
    o.delta_out = peer_delta(peer);
    if (rows == 0) HIP_TRY(hipMemsetAsync(o.delta_out, 0, ntot * sizeof(float), st));
    else if (int e = cd_step_any(ctx, 3, v_pieces, p, mirror, mirror_bytes, v_batch, rows, ldv, &o, 7, workspace, workspace_bytes, stream)) return e;
    PeerSrc src;
    if (int e = peer_exchange_shot1(peer, ctx->status, st, &src)) return e;
    // shot 2 = the apply: the packed total as ONE "slab" whose rows come from the band owners, one row of bias sums each
    const Mirror m = carve_mirror(&ctx->plan, mirror, p->n_vis, p->n_hid, 3);
    ReduceArgs a;
    memset(&a, 0, sizeof a);
    a.slab = src.own_sum; a.slab_stride = 0; a.nslab = 1; a.ld_slab = p->n_hid;
    a.n_vis = p->n_vis; a.n_hid = p->n_hid; a.ldw = p->ldw; a.lr = o.lr;
    a.W = p->W;
    a.part_h = src.own_sum + nw; a.nrow_tiles_h = 1; a.ld_part_h = p->n_hid; a.b_h = p->b_h;
    a.part_v = src.own_sum + nw + p->n_hid; a.nrow_tiles_v = 1; a.ld_part_v = p->n_vis; a.b_v = p->b_v;
    a.Wb = m.Wb; a.ldWb = m.ldW; a.planeWb = m.planeW;
    a.Wtb = m.Wtb; a.ldWtb = m.ldWt; a.planeWtb = m.planeWt; a.pieces = 3;
    a.tile_rows = knob(ctx, KN_REDUCE_TR);
    HIP_TRY(launch_reduce_apply_split(a, st, &src));
    return KURBM_OK;
}

int kurbm_cd_step_x3_dp(kurbm_ctx* ctx, kurbm_comm* comm, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                        const float* v_batch, int v_pieces, int rows, int ldv, const kurbm_cd_opts* opts, int n_chunks,
                        void* workspace, size_t workspace_bytes, kurbm_stream_t stream) {
    return cd_step_dp_any(ctx, comm, 3, p, mirror, mirror_bytes, v_batch, v_pieces, rows, ldv, opts, n_chunks, workspace, workspace_bytes, stream);
}

int kurbm_cd_step_bf16_dp(kurbm_ctx* ctx, kurbm_comm* comm, const kurbm_params* p, void* mirror, size_t mirror_bytes,
                          const float* v_batch, int rows, int ldv, const kurbm_cd_opts* opts, int n_chunks, void* workspace,
                          size_t workspace_bytes, kurbm_stream_t stream) {
    return cd_step_dp_any(ctx, comm, 1, p, mirror, mirror_bytes, v_batch, 1, rows, ldv, opts, n_chunks, workspace, workspace_bytes, stream);
}

}  // extern "C"
