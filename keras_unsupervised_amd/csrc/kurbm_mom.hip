// kurbm_mom.hip -- the MOM instantiations of the reduce / apply launches: momentum and L2 weight decay fused into the launch that
// applies the update (include/kurbm.h: kurbm_momentum; the rule: kurbm_kernels.h, MomArgs; the bodies: kurbm_reduce.h).  A file
// of its own: a run that never asks for momentum never loads this code object, and those of the other files are unchanged.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kurbm_kernels.h"
#include "kurbm_device.h"
#include "kurbm_reduce.h"

namespace kurbm {

// x3 / bf16 steps and the one-launch apply after an exchange
template <int TR>
__global__ __launch_bounds__(256) void k_reduce_apply_split_mom(ReduceArgs a, int tiles_x, int tiles, int nbias, MomArgs mo) {
    warm_kernel_arguments<sizeof(ReduceArgs) + 16 + sizeof(MomArgs)>();
    PeerSrc none;
    none.band_rows = 0;
    reduce_apply_split_body<TR, false, true>(a, tiles_x, tiles, nbias, none, mo);
}

// fp32 step, and the two-launch form of the x3 / bf16 steps (n_hid % 4 != 0)
__global__ __launch_bounds__(256) void k_reduce_apply_mom(ReduceArgs a, int nbias, int nbias8, MomArgs mo) {
    warm_kernel_arguments<sizeof(ReduceArgs) + 8 + sizeof(MomArgs)>();
    reduce_apply_body<true>(a, mo, nbias, nbias8);
}


// params += vel for a packed [V*H | H | V] delta (the velocity of element q is at the same offset q)
__global__ __launch_bounds__(256) void k_apply_delta_mom(ApplyArgs a, MomArgs mo) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nw = (long long)a.n_vis * a.n_hid;
    if (q < nw) {
        if (a.W) {
            const int i = (int)(q / a.n_hid), j = (int)(q - (long long)i * a.n_hid);
            mom_w1(a.W + (size_t)i * a.ldw + j, mo.vel_w + q, a.delta[q], a.lr, mo);
        }
    } else if (q < nw + a.n_hid) {
        if (a.b_h) { const float v = mo.mu * mo.vel_bh[q - nw] + a.lr * a.delta[q]; mo.vel_bh[q - nw] = v; a.b_h[q - nw] += v; }
    } else if (q < nw + a.n_hid + a.n_vis) {
        const long long c = q - nw - a.n_hid;
        if (a.b_v) { const float v = mo.mu * mo.vel_bv[c] + a.lr * a.delta[q]; mo.vel_bv[c] = v; a.b_v[c] += v; }
    }
}

hipError_t launch_reduce_apply_split_mom(const ReduceArgs& a, hipStream_t st, int tr, int tiles_x, int tiles, int nb, const MomArgs& mo) {
    const dim3 grid(tiles + nb);
    if (tr == 64) hipLaunchKernelGGL(k_reduce_apply_split_mom<64>, grid, dim3(256), 0, st, a, tiles_x, tiles, nb, mo);
    else if (tr == 32) hipLaunchKernelGGL(k_reduce_apply_split_mom<32>, grid, dim3(256), 0, st, a, tiles_x, tiles, nb, mo);
    else hipLaunchKernelGGL(k_reduce_apply_split_mom<16>, grid, dim3(256), 0, st, a, tiles_x, tiles, nb, mo);
    return hipGetLastError();
}

hipError_t launch_reduce_apply_mom(const ReduceArgs& a, hipStream_t st, int nb, int nb8, const MomArgs& mo) {
    hipLaunchKernelGGL(k_reduce_apply_mom, dim3(a.nblk_w + nb8), dim3(256), 0, st, a, nb, nb8, mo);
    return hipGetLastError();
}

hipError_t launch_apply_delta_mom(const ApplyArgs& a, hipStream_t st, const MomArgs& mo) {
    const long long n = (long long)a.n_vis * a.n_hid + a.n_hid + a.n_vis;
    hipLaunchKernelGGL(k_apply_delta_mom, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, mo);
    return hipGetLastError();
}

}  // namespace kurbm
