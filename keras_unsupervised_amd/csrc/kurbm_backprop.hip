// kurbm_backprop.hip -- the activation-derivative site of a layer's backward pass when a DBN is fine-tuned on sum log p(y | v)
// (k_backprop_delta), and the fixed-order sum of its row-tile partials into the packed delta (k_backprop_reduce).
// include/kurbm.h, "fine-tuning a DBN", states the model.
//
// Layer l is given e = dL/dx_l [rows][n_hid] and its own output x = x_l = act(x_{l-1}.W + b_h), the plane the forward half step left:
//     delta = e * act'(x)          sigmoid: x (1 - x)      relu: [x > 0]  (a select: exact)      linear: 1  (delta = e, x is not read)
//     db_h[j] = sum_rows delta[.][j]
// The two GEMMs around the site are the existing fp32 launches: dW = x_{l-1}^T.delta is the one-segment statistics GEMM, and
// e_{l-1} = delta.W^T the linear h -> v half step with a zero bias (the db_v block of the packed delta, which k_backprop_reduce has
// just zeroed).  No random number is drawn, nothing is atomic, every sum runs in one fixed order: both kernels are bit-reproducible,
// and a row's delta does not depend on how many rows share the launch.
//
// k_backprop_delta moves three planes of rows x n_hid floats (e and x read, delta written; two with the linear site) and the tiles'
// partials, one float per BP_ROWS of them; it has no arithmetic to speak of.
//
// What binds the two launches (4096 x 1024, sigmoid, one MI355X: 19.8 us against 8.0 us for a device-to-device copy that moves the
// same 50.3 MB, 2.48 x; profiles/finetune_times.txt): k_backprop_delta itself is memory -- 12.5 us in a kernel trace, 4.0 TB/s, 1.6 x
// the copy, with 16 bytes per thread and access; its grid is 1024 one-wave workgroups, four per CU, each with two round trips to
// memory, so what it lacks against the copy is requests in flight, not width.  The other 7 us are k_backprop_reduce and the gap
// between two launches: 1024 threads that each walk 256 partials are a latency chain, not traffic (1 MB).  With one load per
// addition that chain took 61 us -- a load under a condition is waited for where its branch ends -- which is why its loads go out
// in unconditional batches.  Folding the site into the epilogue of the GEMM in front of it is the follow-up that removes both.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kurbm_kernels.h"
#include "kurbm_device.h"

namespace kurbm {

template <int ACT>
__device__ __forceinline__ float bp_site(float e, float x) {
    if (ACT == ACT_SIGMOID) return e * (x * (1.0f - x));
    if (ACT == ACT_RELU) return x > 0.f ? e : 0.f;
    return e;
}

constexpr int BP_CHUNK = 8;       // rows whose loads are in flight together: 16 requests of 16 bytes per thread

// One workgroup (one wave) per (tile of BP_ROWS rows, slice of BP_COLS hidden columns).  Thread = four adjacent columns j .. j + 3
// (j % 4 == 0; every plane is 16-byte aligned with ld % 4 == 0, so the group is one aligned 16-byte access and a wave's rows are
// contiguous kilobytes); it walks the tile's rows in chunks of BP_CHUNK: all of a chunk's loads first, then the site and the
// stores.  In place (delta == e) a thread has read every element it overwrites before it stores, and no other thread touches
// them.  The four running column sums stay in registers and leave once, to part[tile][j ..].  The last group of a row with
// n_hid % 4 != 0 takes the scalar path: columns [n_hid, ld) are neither loaded nor stored.  Same operations in the same order on
// either path, so a column's numbers do not depend on which one its group took.
template <int ACT>
__global__ __launch_bounds__(BP_THREADS) void k_backprop_delta(BackpropDeltaArgs a) {
    const int tile = blockIdx.x;
    const int row_base = tile * BP_ROWS;
    const int nr = a.rows - row_base < BP_ROWS ? a.rows - row_base : BP_ROWS;
    const int j = (blockIdx.y * BP_THREADS + threadIdx.x) * 4;
    if (j >= a.n_hid) return;
    const float* e = a.e + (size_t)row_base * a.lde + j;
    const float* x = a.x + (size_t)row_base * a.ldx + j;
    float* d = a.delta + (size_t)row_base * a.ldd + j;
    float* pt = a.part + (size_t)tile * a.ld_part + j;
    if (a.n_hid - j >= 4) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int r0 = 0; r0 < nr; r0 += BP_CHUNK) {
            float4 ev[BP_CHUNK], xv[BP_CHUNK];
#pragma unroll
            for (int i = 0; i < BP_CHUNK; ++i) {
                if (r0 + i < nr) {
                    ev[i] = *reinterpret_cast<const float4*>(e + (size_t)(r0 + i) * a.lde);
                    if (ACT != ACT_LINEAR) xv[i] = *reinterpret_cast<const float4*>(x + (size_t)(r0 + i) * a.ldx);
                }
            }
#pragma unroll
            for (int i = 0; i < BP_CHUNK; ++i) {
                if (r0 + i < nr) {
                    float4 o;
                    o.x = bp_site<ACT>(ev[i].x, ACT != ACT_LINEAR ? xv[i].x : 0.f);
                    o.y = bp_site<ACT>(ev[i].y, ACT != ACT_LINEAR ? xv[i].y : 0.f);
                    o.z = bp_site<ACT>(ev[i].z, ACT != ACT_LINEAR ? xv[i].z : 0.f);
                    o.w = bp_site<ACT>(ev[i].w, ACT != ACT_LINEAR ? xv[i].w : 0.f);
                    s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
                    *reinterpret_cast<float4*>(d + (size_t)(r0 + i) * a.ldd) = o;
                }
            }
        }
        *reinterpret_cast<float4*>(pt) = s;
    } else {
        const int nc = a.n_hid - j;      // 1 .. 3
        float s[3] = {0.f, 0.f, 0.f};
        for (int r = 0; r < nr; ++r) {
            float ev[3], xv[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c < nc) {
                    ev[c] = e[(size_t)r * a.lde + c];
                    xv[c] = ACT != ACT_LINEAR ? x[(size_t)r * a.ldx + c] : 0.f;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c < nc) {
                    const float o = bp_site<ACT>(ev[c], xv[c]);
                    s[c] += o;
                    d[(size_t)r * a.ldd + c] = o;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (c < nc) pt[c] = s[c];
    }
}

hipError_t launch_backprop_delta(const BackpropDeltaArgs& a, hipStream_t st) {
    if (a.rows < 1 || a.n_hid < 1) return hipErrorInvalidValue;
    const dim3 grid((a.rows + BP_ROWS - 1) / BP_ROWS, (a.n_hid + BP_COLS - 1) / BP_COLS);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    if (a.act == ACT_SIGMOID) hipLaunchKernelGGL(k_backprop_delta<ACT_SIGMOID>, grid, dim3(BP_THREADS), 0, st, a);
    else if (a.act == ACT_RELU) hipLaunchKernelGGL(k_backprop_delta<ACT_RELU>, grid, dim3(BP_THREADS), 0, st, a);
    else if (a.act == ACT_LINEAR) hipLaunchKernelGGL(k_backprop_delta<ACT_LINEAR>, grid, dim3(BP_THREADS), 0, st, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// The tiles' partials -> db_h, tiles in index order, the sum in double and rounded once (the idiom of k_class_reduce); one thread
// per hidden unit, and one per visible unit for the zeros of db_v (nullable: the site's test hook has no packed delta).  A thread's
// loads go out BPR_BATCH at a time before the additions that consume them, in order: one load per addition made the walk a chain of
// memory latencies, 256 of them at 4096 rows -- and a load under a condition is waited for where its branch ends, so a batch's loads
// are unconditional (a tile past the end re-reads the last one and adds 0.0, which changes no sum).
constexpr int BPR_THREADS = 64, BPR_BATCH = 32;
__global__ __launch_bounds__(BPR_THREADS) void k_backprop_reduce(BackpropReduceArgs a) {
    const int t = blockIdx.x * BPR_THREADS + threadIdx.x;
    if (t < a.n_hid) {
        const float* src = a.part + t;
        const int last = a.ntiles - 1;
        double s = 0.;
        for (int k0 = 0; k0 < a.ntiles; k0 += BPR_BATCH) {
            float x[BPR_BATCH];
#pragma unroll
            for (int i = 0; i < BPR_BATCH; ++i) x[i] = src[(size_t)(k0 + i < a.ntiles ? k0 + i : last) * a.ld_part];
#pragma unroll
            for (int i = 0; i < BPR_BATCH; ++i) s += k0 + i < a.ntiles ? (double)x[i] : 0.;
        }
        a.db_h[t] = (float)s;
    } else if (a.db_v && t - a.n_hid < a.n_vis) {
        a.db_v[t - a.n_hid] = 0.f;
    }
}

hipError_t launch_backprop_reduce(const BackpropReduceArgs& a, hipStream_t st) {
    if (a.n_hid < 1 || a.ntiles < 1) return hipErrorInvalidValue;
    const long long n = (long long)a.n_hid + (a.db_v ? a.n_vis : 0);
    hipLaunchKernelGGL(k_backprop_reduce, dim3((unsigned)((n + BPR_THREADS - 1) / BPR_THREADS)), dim3(BPR_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace kurbm
