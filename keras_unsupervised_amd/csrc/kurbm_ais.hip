// kurbm_ais.hip -- the small launches of an annealed-importance-sampling run (kurbm_ais_run, kurbm_ais_step).
//
// The two GEMM launches of a temperature are EPI_AIS of k_gemm (kurbm_kernels.hip); here is what goes around them: the start of
// the chains (v_0 and its bias dot product) and the step that adds a temperature's row partials into log w.  Every sum runs in
// one fixed order and nothing is atomic: a run is bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kurbm_kernels.h"
#include "kurbm_device.h"

namespace kurbm {

// One wave per chain.  draw: v[row][c] = [u < sigmoid(b_A[c])], u = the Philox uniform of (row0 + row, c) at the launch's site;
// else v is read.  vpart[row] = sum_c (b_v - b_A)[c] v[row][c]: lane l adds columns l, l + 64, ... in order, then an xor tree.
__global__ __launch_bounds__(256) void k_ais_start(float* __restrict__ v, int ldv, const float* __restrict__ b_v,
                                                   const float* __restrict__ base_bias, float* __restrict__ vpart,
                                                   double* __restrict__ logw, int rows, int n_vis, int draw, RngArgs rng) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const uint64_t grow = rng.row0 + (uint64_t)row;
    const int word = (int)(grow & 3);
    float t = 0.f;
    for (int c = lane; c < n_vis; c += 64) {
        const float ba = base_bias[c];
        float x;
        if (draw) {
            uint32_t w[4];
            philox4x32_10((uint32_t)c, (uint32_t)(grow >> 2), rng.stream_id, rng.step, rng.seed_lo, rng.seed_hi, w);
            const uint32_t wr = word == 0 ? w[0] : (word == 1 ? w[1] : (word == 2 ? w[2] : w[3]));
            x = (u32_to_unit(wr) < sigmoidf_fast(ba)) ? 1.0f : 0.0f;
            v[(size_t)row * ldv + c] = x;
        } else {
            x = v[(size_t)row * ldv + c];
        }
        t += (b_v[c] - ba) * x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (lane == 0) {
        vpart[row] = t;
        if (logw) logw[row] = 0.0;
    }
}

// part[0 .. ng)[row] added in index order.  Sixteen loads are in flight before the first add: as one load per add the 64 + 49
// groups of a 784 x 1024 model were 113 dependent memory latencies, 26 us of an 82 us temperature.  (The zeros that pad the last
// batch change no sum.)
__device__ __forceinline__ float group_sum(const float* __restrict__ part, int ng, int ld_part, int row) {
    float s = 0.f;
    for (int i0 = 0; i0 < ng; i0 += 16) {
        float x[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) x[e] = part[(size_t)(i0 + e < ng ? i0 + e : ng - 1) * ld_part + row];   // (branch-free loads)
#pragma unroll
        for (int e = 0; e < 16; ++e) s += (i0 + e < ng) ? x[e] : 0.f;
    }
    return s;
}

// One thread per chain: Delta =dbeta (b_v - b_A).v + sum_j [softplus(beta a_j) - softplus(beta_prev a_j)] from the row partials
// of the two GEMM launches (groups of 16 columns, added in index order), into the chain's log w in double.
__global__ __launch_bounds__(256) void k_ais_accumulate(const float* __restrict__ sppart, int ng_sp, const float* __restrict__ vpart,
                                                        int ng_v, int ld_part, float dbeta, double* __restrict__ logw,
                                                        float* __restrict__ dlogw, int rows) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const float s = group_sum(sppart, ng_sp, ld_part, row), d = group_sum(vpart, ng_v, ld_part, row);
    const float delta = fmaf(dbeta, d, s);
    if (logw) logw[row] += (double)delta;
    if (dlogw) dlogw[row] = delta;
}

hipError_t launch_ais_start(float* v, int ldv, const float* b_v, const float* base_bias, float* vpart, double* logw, int rows,
                            int n_vis, int draw, const RngArgs& rng, hipStream_t st) {
    hipLaunchKernelGGL(k_ais_start, dim3((rows + 3) / 4), dim3(256), 0, st, v, ldv, b_v, base_bias, vpart, logw, rows, n_vis, draw, rng);
    return hipGetLastError();
}

hipError_t launch_ais_accumulate(const float* sppart, int ng_sp, const float* vpart, int ng_v, int ld_part, float dbeta,
                                 double* logw, float* dlogw, int rows, hipStream_t st) {
    hipLaunchKernelGGL(k_ais_accumulate, dim3((rows + 255) / 256), dim3(256), 0, st, sppart, ng_sp, vpart, ng_v, ld_part, dbeta,
                       logw, dlogw, rows);
    return hipGetLastError();
}

}  // namespace kurbm
