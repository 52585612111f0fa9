// kurbm_classgrad.hip -- the discriminative gradient of a label RBM: the operands of d log p(y | v) / d theta from the pre-activation
// plane and the class posterior (k_class_grad), and the fixed-order sum of its row-tile partials into the packed delta
// (k_class_reduce).  include/kurbm.h, "discriminative and hybrid training", states the model.
//
// With a = v_pix.W[:n_pix] + b_h (the linear half step kurbm_class_logits already runs), U = W[n_pix:], o_cj = a_j + U_cj,
// p = softmax(logit) from k_class_logits, t the one-hot block of the row and y its class, q = t - p:
//     S_y[j] = sigmoid(o_yj)      H_bar[j] = sum_c p_c sigmoid(o_cj)      g_j = S_y[j] - H_bar[j]
//     nll    = logsumexp_c(logit) - logit_y            (from the LOGITS: finite where p_y has underflowed to zero)
//     dU[c][j] = sum_rows q_c sigmoid(o_cj)       db_h[j] = sum_rows g_j       dd[c] = sum_rows q_c
// The pixel rows of dW, v_pix^T.S_y - v_pix^T.H_bar = v_pix^T.g, are the statistics GEMM's on the ONE plane g (k_gemm unchanged: its
// k walk takes one segment as it stands), half the work of the two-segment form; S_y and H_bar leave only when a caller asks.
// No random number is drawn, nothing is atomic, every sum runs in one fixed order: both kernels are bit-reproducible, and a row's
// S_y, H_bar and nll do not depend on how many rows share the launch.
//
// What binds k_class_grad (794 x 1024, C = 10, 4096 rows, one MI355X: 33.2 us, profiles/disc_times.txt): rows n_hid C = 41.9 M sigmoids
// of one v_exp_f32 and one v_rcp_f32 each, against two planes of rows x n_hid floats (a read, g written: 33.6 MB).  Measured, it is
// not memory: 1.0 TB/s is a sixth of what the device sustains from HBM, and writing S_y and H_bar as well (half as much traffic
// again) took the same 33.2 us.  It is the vector unit's instruction ISSUE, of which the transcendentals are a part and not the
// whole: 33.2 us at 2.4 GHz on 256 CUs x 4 SIMDs x 16 lanes is 31 lane-cycles per sigmoid, for the 17 instructions the inner loop spends on one
// (the add, the scale by log2 e, v_exp, the + 1, v_rcp, two fused multiply-adds, the select for S_y, the LDS reads of p and q and
// their waits).  It is a third of the statistics launches behind it (104 us) and an eighth of the step (256 us), whose larger
// parts are the unchanged half step + k_class_logits (115 us) and that GEMM.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kurbm_kernels.h"
#include "kurbm_device.h"

namespace kurbm {

// One workgroup per (tile of CG_ROWS rows, slice of CG_THREADS hidden columns).  Thread = one hidden column j: U[c][j] and the C
// running dU sums stay in registers, the lanes' loads of a[r][j ..] and their stores of g (and of S_y, H_bar where given) are coalesced, p[r][.],
// q[r][.] and y[r] are wave-uniform reads of LDS.  The tile's partials leave once, at the end:
//     part[tile][c][j] (c < C) = the tile's dU[c][j], rows in order;   part[tile][C][j] = its db_h[j]
//     part_d[tile][c] = its dd[c]  (column slice 0; one thread per class, rows in order)
// nll is written by column slice 0, one thread per row.  32 rows x 256 columns: 4096 x 1024 is 512 workgroups of four waves,
// eight waves per CU on 256 CUs.
template <int CMAX>
__global__ __launch_bounds__(CG_THREADS) void k_class_grad(ClassGradArgs a) {
    __shared__ float p_s[CG_ROWS][CMAX];
    __shared__ float q_s[CG_ROWS][CMAX];
    __shared__ int y_s[CG_ROWS];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const int row_base = tile * CG_ROWS;
    const int nr = a.rows - row_base < CG_ROWS ? a.rows - row_base : CG_ROWS;
    const int C = a.C;

    if (tid < nr) {
        // the first unit of the block that is on (fit() has checked the block: exactly one is); none: the last class, as the label site
        const float* __restrict__ t = a.v + (size_t)(row_base + tid) * a.ldv + a.n_pix;
        int y = C - 1;
        for (int c = C - 1; c >= 0; --c)
            if (t[c] > 0.5f) y = c;
        y_s[tid] = y;
    }
    __syncthreads();
    for (int i = tid; i < nr * C; i += CG_THREADS) {
        const int r = i / C, c = i - r * C;
        const float p = a.prob[(size_t)(row_base + r) * a.ldl + c];
        p_s[r][c] = p;
        q_s[r][c] = (c == y_s[r] ? 1.0f : 0.0f) - p;
    }
    __syncthreads();

    const int j = blockIdx.y * CG_THREADS + tid;
    if (j < a.n_hid) {
        float U[CMAX], dU[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            U[c] = c < C ? a.W[(size_t)(a.n_pix + c) * a.ldw + j] : 0.f;
            dU[c] = 0.f;
        }
        float dbh = 0.f;
        for (int r = 0; r < nr; ++r) {
            const size_t row = (size_t)(row_base + r);
            const float aj = a.a[row * a.lda + j];
            const int y = y_s[r];
            float sy = 0.f, hb = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                if (c < C) {
                    const float s = sigmoidf_fast(aj + U[c]);
                    hb = fmaf(p_s[r][c], s, hb);
                    dU[c] = fmaf(q_s[r][c], s, dU[c]);
                    sy = (c == y) ? s : sy;
                }
            }
            const float gj = sy - hb;
            dbh += gj;
            a.g[row * a.ldg + j] = gj;
            if (a.S_y) a.S_y[row * a.ldh + j] = sy;         // (uniform over the launch)
            if (a.H_bar) a.H_bar[row * a.ldh + j] = hb;
        }
        float* __restrict__ pt = a.part + (size_t)tile * (C + 1) * a.ld_part + j;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) pt[(size_t)c * a.ld_part] = dU[c];
        pt[(size_t)C * a.ld_part] = dbh;
    }

    if (blockIdx.y == 0) {
        if (tid < C) {
            float t = 0.f;
            for (int r = 0; r < nr; ++r) t += q_s[r][tid];
            a.part_d[(size_t)tile * CG_PART_D + tid] = t;
        } else if (tid >= 64 && tid < 64 + nr) {      // (the second wave: C <= 64 keeps the two jobs apart)
            const int r = tid - 64;
            const float* __restrict__ lg = a.logits + (size_t)(row_base + r) * a.ldl;
            float m = lg[0];
            for (int c = 1; c < C; ++c) m = fmaxf(m, lg[c]);
            float s = 0.f;
            for (int c = 0; c < C; ++c) s += expf(lg[c] - m);
            a.nll[row_base + r] = (m - lg[y_s[r]]) + logf(s);
        }
    }
}

hipError_t launch_class_grad(const ClassGradArgs& a, hipStream_t st) {
    if (a.rows < 1 || a.C < 2 || a.C > 64 || a.n_hid < 1) return hipErrorInvalidValue;
    const dim3 grid((a.rows + CG_ROWS - 1) / CG_ROWS, (a.n_hid + CG_THREADS - 1) / CG_THREADS);
    if (a.C <= 16) hipLaunchKernelGGL(k_class_grad<16>, grid, dim3(CG_THREADS), 0, st, a);
    else hipLaunchKernelGGL(k_class_grad<64>, grid, dim3(CG_THREADS), 0, st, a);
    return hipGetLastError();
}

// a + w * g with the product ROUNDED before the sum (the header's definition of the hybrid delta; hipcc contracts a * b + c into an
// fma by default, and its __fmul_rn / __fadd_rn are plain operators that contract just the same)
__device__ __forceinline__ float add_rounded_product(float a, float w, float g) {
#pragma clang fp contract(off)
    const float prod = w * g;
    return a + prod;
}

// The tiles' partials -> the packed delta [dW | db_h | db_v], tiles in index order, each sum in double and rounded once.  One thread per
// element of the TAIL -- rows n_pix .. of dW, db_h, db_v (zeros in db_v[:n_pix]) -- and, with a generative delta, one more per element
// of the pixel rows of dW, which the statistics launch in front has already written: everywhere delta = disc + gen_weight * gen, the
// product rounded before the sum.  Block 0 alone writes the batch's mean nll (nullable): 256 strided double sums, then a fixed tree.
__global__ __launch_bounds__(256) void k_class_reduce(ClassReduceArgs a) {
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {
        if (!a.nll_mean) return;     // (uniform over the block)
        __shared__ double red[256];
        double s = 0.;
        for (int r = tid; r < a.rows; r += 256) s += (double)a.nll[r];
        red[tid] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) *a.nll_mean = (float)(red[0] / (double)a.rows);
        return;
    }
    const int C = a.C, n_hid = a.n_hid, n_vis = a.n_pix + C;
    const size_t nw = (size_t)n_vis * n_hid, n_pixw = (size_t)a.n_pix * n_hid;
    const size_t tail = (size_t)(C + 1) * n_hid + n_vis;
    const size_t t = (size_t)(blockIdx.x - 1) * 256 + tid;
    size_t out;
    float v;
    if (t < tail) {
        const float* src;
        size_t stride;
        if (t < (size_t)(C + 1) * n_hid) {
            const int c = (int)(t / n_hid), j = (int)(t - (size_t)c * n_hid);
            src = a.part + (size_t)c * a.ld_part + j;
            stride = (size_t)(C + 1) * a.ld_part;
            out = c < C ? n_pixw + t : nw + j;
        } else {
            const int i = (int)(t - (size_t)(C + 1) * n_hid);
            src = i >= a.n_pix ? a.part_d + (i - a.n_pix) : nullptr;
            stride = CG_PART_D;
            out = nw + n_hid + i;
        }
        double s = 0.;
        if (src)
            for (int k = 0; k < a.ntiles; ++k) s += (double)src[(size_t)k * stride];
        v = (float)s;
    } else {
        out = t - tail;
        if (!a.gen || out >= n_pixw) return;
        v = a.delta[out];
    }
    if (a.gen) v = add_rounded_product(v, a.gen_weight, a.gen[out]);
    a.delta[out] = v;
}

hipError_t launch_class_reduce(const ClassReduceArgs& a, hipStream_t st) {
    const size_t n_vis = (size_t)a.n_pix + a.C;
    size_t n = (size_t)(a.C + 1) * a.n_hid + n_vis;
    if (a.gen) n += (size_t)a.n_pix * a.n_hid;
    const size_t blocks = 1 + (n + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_class_reduce, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace kurbm
