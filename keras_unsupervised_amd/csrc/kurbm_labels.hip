// kurbm_labels.hip -- softmax label units: the categorical sampling site of the label block (k_label_sample) and the class
// logits of a label RBM (k_class_logits).  include/kurbm.h, "softmax label units", states both.
//
// A label RBM keeps its C label units in the LAST C visible columns: rows n_pix .. n_vis-1 of W (contiguous in memory) and
// entries n_pix .. of b_v.  The h -> v half step treats them as Bernoulli units like every other column; k_label_sample runs
// behind it and rewrites the block as ONE draw of softmax(b_v + h.W^T).  Every sum here runs in one fixed order and nothing is
// atomic: both kernels are bit-reproducible, and a row's numbers do not depend on how many rows share the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kurbm_kernels.h"
#include "kurbm_device.h"

namespace kurbm {

constexpr int LBL_LD = 65;              // LDS row stride of x: consecutive rows start in consecutive banks
constexpr int LBL_ROWS = 128;           // most rows per workgroup (the tallest tile of the half step)
constexpr int LBL_THREADS = 512;

// Four floats of a row from element k on; zeros where the row is not to be read (`ok`) and from n_hid on (k % 4 == 0 and the leading
// dimensions are multiples of 4, so the 16 bytes lie inside the row -- but what they hold beyond n_hid is padding, NaN in the tests).
__device__ __forceinline__ f32x4 lbl_load4(const float* __restrict__ p, bool ok, int k, int n_hid) {
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (ok && k < n_hid) {
        x = *reinterpret_cast<const f32x4*>(p + k);
        if (k + 1 >= n_hid) x[1] = 0.f;
        if (k + 2 >= n_hid) x[2] = 0.f;
        if (k + 3 >= n_hid) x[3] = 0.f;
    }
    return x;
}

// One workgroup per `tile_h` rows (the row tile of the h -> v launch in front; <= 128), 8 waves; wave w owns rows 16 w .. 16 w + 15
// of the tile and all classes, in NB blocks of 16 (NB = 1: C <= 16; NB = 4: C <= 64).
//   x_c = b_v[n_pix + c] + sum_j h_j W[n_pix + c][j] on v_mfma_f32_16x16x4_f32 (exact fp32 fma chains, as the half steps use it):
//         lane (m, g) = (lane & 15, lane >> 4) reads 16 bytes of row m of h and of label row 16 cb + m of W at k + 4 g -- both
//         straight from memory into the operand registers (the rows are contiguous and nobody else in the workgroup needs them),
//         the next 64 hidden units in flight under the matrix instructions of these -- and element e of the two is one operand
//         pair; the order of the additions is fixed by k and the instruction alone.  (No operand goes through LDS: each is read
//         by exactly one lane, so staging would add LDS traffic and barriers and save no memory traffic.)
//   then ONE thread per row: m = max x; e_c = exp(x_c - m); s = sum e_c in class order; p_c = e_c / s; the drawn class is the first
//         c with u < p_0 + .. + p_c (running fp32 sum in class order), else C - 1; u = the Philox uniform of (row0 + row, n_pix).
//   the block v[row][n_pix ..] becomes that one-hot vector; prob / out_u (nullable) receive p and u.
//   part (nullable): part[blockIdx.x][n_pix + c] = sum over the tile's rows, in row order, of ref[row][n_pix + c] - v[row][n_pix + c]
//         (small integers: exact), the label columns of the half step's visible-bias partials.
template <int NB>
__global__ __launch_bounds__(LBL_THREADS) void k_label_sample(LabelArgs a) {
    __shared__ float xs[LBL_ROWS * LBL_LD];      // the pre-activations x [row][class]
    __shared__ int cls_s[LBL_ROWS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 15, g = lane >> 4;
    const int row_base = blockIdx.x * a.tile_h;
    const int C = a.C, n_hid = a.n_hid;

    if (wave * 16 < a.tile_h) {      // (wave-uniform; no barrier inside)
        const int rt = wave * 16 + m;
        const bool a_ok = rt < a.tile_h && row_base + rt < a.rows;
        const float* __restrict__ ha = a.h + (size_t)(a_ok ? row_base + rt : 0) * a.ldh;
        const float* __restrict__ wb[NB];
        bool b_ok[NB];
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
            b_ok[cb] = 16 * cb + m < C;           // (label rows end with W: nothing behind row n_vis - 1 is read)
            wb[cb] = a.W + (size_t)(a.n_pix + (b_ok[cb] ? 16 * cb + m : 0)) * a.ldw;
        }
        f32x4 acc[NB];
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 A0[4], A1[4], B0[4][NB], B1[4][NB];
        // hidden units k0 .. k0 + 63, all below n_hid: unconditional loads, nothing looks at a value before the matrix instructions
        // do (a lane without a row or a class of its own reads row / class 0: its products land in rows / columns nobody reads)
        auto fetch = [&](f32x4 (&A)[4], f32x4 (&B)[4][NB], int k0) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = k0 + 16 * s + 4 * g;
                A[s] = *reinterpret_cast<const f32x4*>(ha + k);
#pragma unroll
                for (int cb = 0; cb < NB; ++cb) B[s][cb] = *reinterpret_cast<const f32x4*>(wb[cb] + k);
            }
        };
        // the last n_hid % 64 units: guarded loads, zeros from n_hid on
        auto fetch_tail = [&](f32x4 (&A)[4], f32x4 (&B)[4][NB], int k0) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = k0 + 16 * s + 4 * g;
                A[s] = lbl_load4(ha, a_ok, k, n_hid);
#pragma unroll
                for (int cb = 0; cb < NB; ++cb) B[s][cb] = lbl_load4(wb[cb], b_ok[cb], k, n_hid);
            }
        };
        auto mac = [&](const f32x4 (&A)[4], const f32x4 (&B)[4][NB]) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int cb = 0; cb < NB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[s][e], B[s][cb][e], acc[cb], 0, 0, 0);
        };
        const int n_full = n_hid / 64 * 64;
        if (n_full) {
            // two register sets: the loads of one block are in flight under the matrix instructions of the other.  The loop body has
            // no branch (behind the last pair the prefetch reads the last block again, unused), so the loads stay where they are
            fetch(A0, B0, 0);
            int k0 = 0;
            for (; k0 + 128 <= n_full; k0 += 128) {
                fetch(A1, B1, k0 + 64);
                mac(A0, B0);
                fetch(A0, B0, k0 + 128 < n_full ? k0 + 128 : n_full - 64);
                mac(A1, B1);
            }
            if (k0 < n_full) mac(A0, B0);
        }
        if (n_full < n_hid) {
            fetch_tail(A0, B0, n_full);
            mac(A0, B0);
        }
        // acc[cb][e] = x[row 16 w + 4 g + e][class 16 cb + m]
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
            const int c = 16 * cb + m;
            if (c < C) {
                const float bias = a.b_v[a.n_pix + c];
#pragma unroll
                for (int e = 0; e < 4; ++e) xs[(wave * 16 + 4 * g + e) * LBL_LD + c] = acc[cb][e] + bias;
            }
        }
    }
    __syncthreads();
    if (tid < a.tile_h) {
        const int row = row_base + tid;
        int cls = -1;
        if (row < a.rows) {
            float* x = xs + tid * LBL_LD;
            float m = x[0];
            for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
            float s = 0.f;
            for (int c = 0; c < C; ++c) {
                const float e = expf(x[c] - m);
                x[c] = e;
                s += e;
            }
            const uint64_t grow = a.rng.row0 + (uint64_t)row;
            uint32_t w[4];
            philox4x32_10((uint32_t)a.n_pix, (uint32_t)(grow >> 2), a.rng.stream_id, a.rng.step, a.rng.seed_lo, a.rng.seed_hi, w);
            const int word = (int)(grow & 3);
            const float u = u32_to_unit(word == 0 ? w[0] : (word == 1 ? w[1] : (word == 2 ? w[2] : w[3])));
            float cum = 0.f;
            for (int c = 0; c < C; ++c) {
                const float p = x[c] / s;
                if (a.prob) a.prob[(size_t)row * a.ldp + c] = p;
                cum += p;
                if (cls < 0 && u < cum) cls = c;
            }
            if (cls < 0) cls = C - 1;
            if (a.out_u) a.out_u[row] = u;
            float* vr = a.v + (size_t)row * a.ldv + a.n_pix;
            for (int c = 0; c < C; ++c) vr[c] = (c == cls) ? 1.0f : 0.0f;
        }
        cls_s[tid] = cls;
    }
    if (a.part) {      // (uniform over the launch)
        __syncthreads();
        if (tid < C) {
            float t = 0.f;
            for (int rr = 0; rr < a.tile_h; ++rr) {
                const int row = row_base + rr;
                if (row < a.rows) t += a.ref[(size_t)row * a.ldref + a.n_pix + tid] - (cls_s[rr] == tid ? 1.0f : 0.0f);
            }
            a.part[(size_t)blockIdx.x * a.ld_part + a.n_pix + tid] = t;
        }
    }
}

hipError_t launch_label_sample(const LabelArgs& a, hipStream_t st) {
    // the kernel's LDS and its row-to-wave mapping hold LBL_ROWS rows: a taller tile is an error here, not an overrun there
    if (a.tile_h < 1 || a.tile_h > LBL_ROWS || a.C < 2 || a.C > 64) return hipErrorInvalidValue;
    const int grid = (a.rows + a.tile_h - 1) / a.tile_h;
    if (a.C <= 16) hipLaunchKernelGGL(k_label_sample<1>, dim3(grid), dim3(LBL_THREADS), 0, st, a);
    else hipLaunchKernelGGL(k_label_sample<4>, dim3(grid), dim3(LBL_THREADS), 0, st, a);
    return hipGetLastError();
}

// One wave per row.  a [rows][lda] = v.W[:n_pix] + b_h (the linear half step on the pixel rows of W).  Lane l walks hidden units
// l, l + 64, ...: it reads a_j ONCE and adds softplus(a_j + W[n_pix + c][j]) into one register per class; the 64 lane sums of a
// class meet in an xor-shuffle tree.  logit_c = b_v[n_pix + c] + that sum; prob (nullable) = softmax(logit) over the classes.
template <int CMAX>
__global__ __launch_bounds__(256) void k_class_logits(ClassLogitArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    if (row >= a.rows) return;
    const int C = a.C;
    const float* __restrict__ Wl = a.W + (size_t)a.n_pix * a.ldw;
    const float* __restrict__ ar = a.a + (size_t)row * a.lda;
    float acc[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) acc[c] = 0.f;
    for (int j = lane; j < a.n_hid; j += 64) {
        const float aj = ar[j];
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) acc[c] += softplusf(aj + Wl[(size_t)c * a.ldw + j]);
    }
    float mine = -INFINITY;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        if (c < C) {
            float t = acc[c];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
            if (lane == c) mine = t + a.b_v[a.n_pix + c];
        }
    }
    if (lane < C) a.logits[(size_t)row * a.ldl + lane] = mine;
    if (a.prob) {
        float m = mine;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        const float e = lane < C ? expf(mine - m) : 0.f;
        float s = e;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane < C) a.prob[(size_t)row * a.ldl + lane] = e / s;
    }
}

hipError_t launch_class_logits(const ClassLogitArgs& a, hipStream_t st) {
    const int grid = (a.rows + 3) / 4;
    if (a.C <= 16) hipLaunchKernelGGL(k_class_logits<16>, dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_class_logits<64>, dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace kurbm
