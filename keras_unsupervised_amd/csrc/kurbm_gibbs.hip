// kurbm_gibbs.hip -- the small launches of a Gibbs run (kurbm_gibbs_run).
//
// A sweep is the two x3 half-step launches of kurbm_x3.hip (k_gemm_pb, EPI_HALFSTEP); the chain state stays in their operand
// format -- a k-permuted byte plane for 0/1 visibles, three bf16 pieces for real-valued ones.  Here is what clamping adds: a mask
// in the ORDER OF THE PLANE'S POSITIONS, made once per run, and one launch per sweep that copies the clamped units from the
// converted start plane back into the current plane (and, on a kept sweep, from v_init into the fp32 planes that sweep wrote).
// Plain loads and stores, nothing atomic, nothing summed: a run is bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kurbm_kernels.h"
#include "kurbm_device.h"

namespace kurbm {

typedef uint32_t u32x4g __attribute__((ext_vector_type(4)));

// the column whose byte sits at position p of a k-permuted row (inverse of kperm64: bits 3, 4 of the column are bits 4, 5 of
// the position, bit 5 is bit 3).  Eight positions from a multiple of eight are eight consecutive columns.
__host__ __device__ inline int kperm64_inv(int p) { return (p & ~0x38) | ((p & 0x30) >> 1) | ((p & 0x08) << 2); }

__global__ __launch_bounds__(256) void k_gibbs_mask(const unsigned char* __restrict__ clamp, int n_vis,
                                                    unsigned char* __restrict__ maskp, int npos, int perm) {
    const int pos = blockIdx.x * 256 + threadIdx.x;
    if (pos >= npos) return;
    const int col = perm ? kperm64_inv(pos) : pos;
    maskp[pos] = (col < n_vis && clamp[col] != 0) ? (unsigned char)0xFF : (unsigned char)0;
}

// One thread per (row, 8 positions): most groups of a sparse mask leave after one 8-byte load.
__global__ __launch_bounds__(256) void k_gibbs_clamp(GibbsClampArgs a) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)a.rows * a.ngroups) return;
    const int row = (int)(id / a.ngroups), grp = (int)(id % a.ngroups);
    const uint64_t m = *reinterpret_cast<const uint64_t*>(a.maskp + 8 * grp);
    if (m == 0ull) return;
    const size_t off = (size_t)row * a.ld_bytes + (size_t)8 * grp * a.es;
    for (int j = 0; j < a.pieces; ++j) {
        unsigned char* c = a.cur + (size_t)j * a.plane_bytes + off;
        const unsigned char* s = a.start + (size_t)j * a.plane_bytes + off;
        if (a.es == 1) {
            const uint64_t cv = *reinterpret_cast<const uint64_t*>(c), sv = *reinterpret_cast<const uint64_t*>(s);
            *reinterpret_cast<uint64_t*>(c) = (cv & ~m) | (sv & m);
        } else {   // bf16: mask byte e covers the two bytes of element e
            const u32x4g cv = *reinterpret_cast<const u32x4g*>(c), sv = *reinterpret_cast<const u32x4g*>(s);
            u32x4g o;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const uint32_t md = (((m >> (16 * d)) & 0xFFull) ? 0x0000FFFFu : 0u) | (((m >> (16 * d + 8)) & 0xFFull) ? 0xFFFF0000u : 0u);
                o[d] = (cv[d] & ~md) | (sv[d] & md);
            }
            *reinterpret_cast<u32x4g*>(c) = o;
        }
    }
    if (a.v_out || a.prob_out) {   // a kept sweep: the fp32 planes carry the clamped values too
        const int col0 = a.perm ? kperm64_inv(8 * grp) : 8 * grp;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = col0 + e;
            if (((m >> (8 * e)) & 0xFFull) && col < a.n_vis) {
                const float x = a.v_init[(size_t)row * a.ldv + col];
                if (a.v_out) a.v_out[(size_t)row * a.ldo + col] = x;
                if (a.prob_out) a.prob_out[(size_t)row * a.ldo + col] = x;
            }
        }
    }
}

hipError_t launch_gibbs_mask(const unsigned char* clamp, int n_vis, unsigned char* maskp, int npos, int perm, hipStream_t st) {
    if (npos <= 0 || npos % 8 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gibbs_mask, dim3((npos + 255) / 256), dim3(256), 0, st, clamp, n_vis, maskp, npos, perm);
    return hipGetLastError();
}

hipError_t launch_gibbs_clamp(const GibbsClampArgs& a, hipStream_t st) {
    // (8-byte and 16-byte accesses: the planes' rows and pieces must keep that alignment)
    if ((a.es != 1 && a.es != 2) || a.rows <= 0 || a.ngroups <= 0 || a.ld_bytes % 16 != 0 || a.plane_bytes % 16 != 0)
        return hipErrorInvalidValue;
    const long long n = (long long)a.rows * a.ngroups;
    hipLaunchKernelGGL(k_gibbs_clamp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace kurbm
