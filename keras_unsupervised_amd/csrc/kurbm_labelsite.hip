// kurbm_labelsite.hip -- the softmax label site INSIDE the Gibbs and AIS runs (kurbm_gibbs_run_labels, kurbm_ais_run_labels,
// kurbm_ais_step_labels; include/kurbm.h, "free label blocks"), and the start of an AIS run with a label block.
//
// The site is the one of kurbm_labels.hip (x = bias + h.W_label^T on v_mfma_f32_16x16x4_f32, softmax, one categorical draw per
// row), met in other surroundings:
//   - h is read in the format the run keeps it in: the k-permuted byte plane or one bf16 piece of a Gibbs run, the fp32 plane of an
//     AIS run.  A 0/1 byte or a bf16 0/1 value becomes exactly 0.0f / 1.0f in the operand register, so x is the same fp32 fma chain
//     whatever the format;
//   - the block is written in the format the next launch reads: bytes (0x40 = one) at the k-permuted positions of columns
//     n_pix .. n_vis-1, or bf16 pieces (hi = 1.0 / 0, mid = lo = 0), or fp32 -- and, on a kept sweep, fp32 v_out / prob_out too;
//   - an AIS temperature puts beta and b_A into x, and leaves (b_v - b_A)[n_pix + y] as the row's partial of the label block.
// W is read as its fp32 master rows (the label rows are the LAST rows of W, contiguous), never as the bf16 mirror.
//
// Grid: one 16-row band per workgroup -- rows / 16 workgroups, 256 of them at 4096 chains (one per CU), where the launch of
// kurbm_labels.hip has one workgroup per 128-row tile (32) -- and eight waves per workgroup that share the band's hidden units, so
// that the k loop is one or two rounds of memory latency.  A band reads the C label rows of W once (40 KB at C = 10, n_hid = 1024,
// from L2 after the first band) and n_hid bytes of h per row.
// Cost beside the clamp launch: the clamp launch moves bytes and leaves most groups after one 8-byte load; the site is a GEMM of
// rows x C x n_hid on the fp32 matrix cores followed by a softmax whose sum and draw are serial in the classes by definition, with
// three workgroup barriers between its phases, so it is the slower of the two by construction (README, "free label blocks", has the
// measured times of both).
//
// Every sum runs in one fixed order (k ascending inside a wave's matrix instruction chain, the waves' partial sums in wave order,
// classes in order in the softmax), nothing is atomic, and a row's numbers do not depend on how many rows share the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kurbm_kernels.h"
#include "kurbm_device.h"

namespace kurbm {

constexpr int LS_LD = 65;      // LDS row stride of x: consecutive rows start in consecutive banks
constexpr int LS_ROWS = 16;    // one band
constexpr int LS_WAVES = 8;    // waves of a workgroup: they share the band's hidden units
constexpr int LS_THREADS = 64 * LS_WAVES;

typedef uint32_t u32x2l __attribute__((ext_vector_type(2)));

// Four consecutive hidden units k .. k + 3 (k % 4 == 0) of a row of h as floats; zeros where the row is not to be read and from
// n_hid on.  FMT: LS_H_F32 fp32 [ldh floats]; LS_H_BYTES the k-permuted byte plane [ldh bytes] (kperm64 keeps an aligned group of
// four columns together: one dword); LS_H_BF16 one bf16 piece [ldh elements].
template <int FMT>
__device__ __forceinline__ f32x4 ls_load_h(const void* __restrict__ hrow, bool ok, int k, int n_hid) {
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (ok && k < n_hid) {
        if (FMT == LS_H_F32) {
            x = *reinterpret_cast<const f32x4*>(static_cast<const float*>(hrow) + k);
        } else if (FMT == LS_H_BYTES) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(static_cast<const unsigned char*>(hrow) + kperm64(k));
            x[0] = (w & 0xFFu) ? 1.f : 0.f; x[1] = (w & 0xFF00u) ? 1.f : 0.f;
            x[2] = (w & 0xFF0000u) ? 1.f : 0.f; x[3] = (w & 0xFF000000u) ? 1.f : 0.f;
        } else {
            const u32x2l w = *reinterpret_cast<const u32x2l*>(static_cast<const uint16_t*>(hrow) + k);
            x[0] = __uint_as_float(w[0] << 16); x[1] = __uint_as_float(w[0] & 0xFFFF0000u);
            x[2] = __uint_as_float(w[1] << 16); x[3] = __uint_as_float(w[1] & 0xFFFF0000u);
        }
        if (k + 1 >= n_hid) x[1] = 0.f;
        if (k + 2 >= n_hid) x[2] = 0.f;
        if (k + 3 >= n_hid) x[3] = 0.f;
    }
    return x;
}
__device__ __forceinline__ f32x4 ls_load_w(const float* __restrict__ p, bool ok, int k, int n_hid) {
    return ls_load_h<LS_H_F32>(p, ok, k, n_hid);
}

// One workgroup per 16-row band, LS_WAVES waves; wave w takes the 64-unit blocks w, w + LS_WAVES, ... of the hidden units (at
// n_hid = 1024 two blocks each, both in flight at once: the k loop of a band is ONE round of memory latency, where a single wave
// walking all sixteen blocks, one register set ahead, was sixteen -- 29 us of a 36 us sweep when first measured).
//   lane (m, g) = (lane & 15, lane >> 4) holds row m of the band and label row 16 cb + m of W at k + 4 g: element e of the two loads
//   is one operand pair of the 16x16x4 instruction, as in k_label_sample.  acc[cb][e] = x[row 4 g + e][class 16 cb + m] of the wave's
//   blocks; the waves' partial sums meet in LDS and are added in wave order, so x is a fixed function of (h, W, n_hid).
//   Then, per row: max, exp (one thread per row and class), the sum in class order, p = e / s and the running sum of the draw (one
//   thread per row), and every plane's block (all threads).
template <int NB, int FMT>
__global__ __launch_bounds__(LS_THREADS) void k_label_site(LabelSiteArgs a) {
    __shared__ float ps[LS_WAVES][LS_ROWS * LS_LD];      // the waves' partial pre-activations [row][class]
    __shared__ float xs[LS_ROWS * LS_LD];                // x, later p
    __shared__ float es[LS_ROWS * LS_LD];                // exp(x - max)
    __shared__ float u_s[LS_ROWS];
    __shared__ int cls_s[LS_ROWS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 15, g = lane >> 4;
    const int row_base = blockIdx.x * LS_ROWS;
    const int C = a.C, n_hid = a.n_hid;
    const size_t hes = FMT == LS_H_F32 ? 4 : (FMT == LS_H_BYTES ? 1 : 2);

    const bool a_ok = row_base + m < a.rows;
    const unsigned char* __restrict__ ha = static_cast<const unsigned char*>(a.h) + (size_t)(a_ok ? row_base + m : 0) * a.ldh * hes;
    const float* __restrict__ wb[NB];
    bool b_ok[NB];
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) {
        b_ok[cb] = 16 * cb + m < C;           // (the label rows end with W: nothing behind row n_vis - 1 is read)
        wb[cb] = a.W + (size_t)(a.n_pix + (b_ok[cb] ? 16 * cb + m : 0)) * a.ldw;
    }
    f32x4 acc[NB];
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 A0[4], A1[4], B0[4][NB], B1[4][NB];
    // 64 hidden units from k0 on; every load is guarded (rows past the last one, classes past C and units past n_hid read as zeros:
    // the planes' padding is never let into x)
    auto fetch = [&](f32x4 (&A)[4], f32x4 (&B)[4][NB], int k0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = k0 + 16 * s + 4 * g;
            A[s] = ls_load_h<FMT>(ha, a_ok, k, n_hid);
#pragma unroll
            for (int cb = 0; cb < NB; ++cb) B[s][cb] = ls_load_w(wb[cb], b_ok[cb], k, n_hid);
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
    // two register sets: the loads of one block of 64 are in flight under the matrix instructions of the other (a fetch from
    // n_hid on loads nothing and gives zeros)
    constexpr int STRIDE = 64 * LS_WAVES;
    const int k_first = 64 * wave;
    fetch(A0, B0, k_first);
    fetch(A1, B1, k_first + STRIDE);
    if (wave == LS_WAVES - 1 && lane < LS_ROWS) {      // the rows' uniforms, under the first loads of the wave with the fewest blocks
        const uint64_t grow = a.rng.row0 + (uint64_t)(row_base + lane);
        uint32_t w[4];
        philox4x32_10((uint32_t)a.n_pix, (uint32_t)(grow >> 2), a.rng.stream_id, a.rng.step, a.rng.seed_lo, a.rng.seed_hi, w);
        const int word = (int)(grow & 3);
        u_s[lane] = u32_to_unit(word == 0 ? w[0] : (word == 1 ? w[1] : (word == 2 ? w[2] : w[3])));
    }
    for (int k0 = k_first; k0 < n_hid; k0 += 2 * STRIDE) {
        mac(A0, B0);
        if (k0 + 2 * STRIDE < n_hid) fetch(A0, B0, k0 + 2 * STRIDE);
        if (k0 + STRIDE < n_hid) {
            mac(A1, B1);
            if (k0 + 3 * STRIDE < n_hid) fetch(A1, B1, k0 + 3 * STRIDE);
        }
    }
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) {
        const int c = 16 * cb + m;
        if (c < C) {
#pragma unroll
            for (int e = 0; e < 4; ++e) ps[wave][(4 * g + e) * LS_LD + c] = acc[cb][e];
        }
    }
    __syncthreads();
    const int n_el = LS_ROWS * C;                          // (at most 1024: two turns of the workgroup)
    for (int idx = tid; idx < n_el; idx += LS_THREADS) {
        const int r = idx / C, c = idx - r * C;
        float x = ps[0][r * LS_LD + c];
#pragma unroll
        for (int w = 1; w < LS_WAVES; ++w) x += ps[w][r * LS_LD + c];
        x += a.b_v[a.n_pix + c];
        if (a.base_bias) x = a.one_minus_beta * a.base_bias[a.n_pix + c] + a.beta * x;
        xs[r * LS_LD + c] = x;
    }
    __syncthreads();
    for (int idx = tid; idx < n_el; idx += LS_THREADS) {
        const int r = idx / C, c = idx - r * C;
        const float* x = xs + r * LS_LD;
        float mx = x[0];
        for (int cc = 1; cc < C; ++cc) mx = fmaxf(mx, x[cc]);
        es[r * LS_LD + c] = expf(x[c] - mx);
    }
    __syncthreads();
    if (tid < LS_ROWS) {
        const int row = row_base + tid;
        int cls = -1;
        if (row < a.rows) {
            const float* e = es + tid * LS_LD;
            float* x = xs + tid * LS_LD;
            float s = 0.f;
            for (int c = 0; c < C; ++c) s += e[c];
            const float u = u_s[tid];
            float cum = 0.f;
            for (int c = 0; c < C; ++c) {
                const float p = e[c] / s;
                x[c] = p;
                cum += p;
                if (cls < 0 && u < cum) cls = c;
            }
            if (cls < 0) cls = C - 1;
            if (a.out_u) a.out_u[row] = u;
            if (a.part) a.part[row] = a.b_v[a.n_pix + cls] - a.base_bias[a.n_pix + cls];
        }
        cls_s[tid] = cls;
    }
    __syncthreads();
    // the block of every plane, all threads: element idx = (row of the band, class)
    for (int idx = tid; idx < n_el; idx += LS_THREADS) {
        const int r = idx / C, c = idx - r * C;
        const int row = row_base + r;
        if (row >= a.rows) continue;
        const bool on = cls_s[r] == c;
        const int col = a.n_pix + c;
        if (a.vb) a.vb[(size_t)row * a.ldvb + (size_t)kperm64(col)] = on ? (unsigned char)0x40 : (unsigned char)0;
        if (a.vp) {
            for (int j = 0; j < a.pieces; ++j)
                a.vp[(size_t)j * a.plane + (size_t)row * a.ldvp + col] = (j == 0 && on) ? (uint16_t)0x3F80 : (uint16_t)0;
        }
        if (a.v) a.v[(size_t)row * a.ldv + col] = on ? 1.0f : 0.0f;
        if (a.prob) a.prob[(size_t)row * a.ldp + a.prob_col0 + c] = xs[r * LS_LD + c];
    }
}

template <int NB>
static hipError_t launch_label_site_nb(const LabelSiteArgs& a, hipStream_t st) {
    const dim3 grid((a.rows + LS_ROWS - 1) / LS_ROWS), block(LS_THREADS);
    switch (a.hfmt) {
        case LS_H_F32: hipLaunchKernelGGL((k_label_site<NB, LS_H_F32>), grid, block, 0, st, a); break;
        case LS_H_BYTES: hipLaunchKernelGGL((k_label_site<NB, LS_H_BYTES>), grid, block, 0, st, a); break;
        case LS_H_BF16: hipLaunchKernelGGL((k_label_site<NB, LS_H_BF16>), grid, block, 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_label_site(const LabelSiteArgs& a, hipStream_t st) {
    // the loads are 4, 8 and 16 bytes wide: the rows of every plane must keep that alignment
    if (a.rows <= 0 || a.C < 2 || a.C > 64 || a.n_pix < 1 || a.n_hid < 1 || !a.h || !a.W || !a.b_v || a.ldh % 4 != 0 || a.ldw % 4 != 0)
        return hipErrorInvalidValue;
    if (a.part && !a.base_bias) return hipErrorInvalidValue;
    return a.C <= 16 ? launch_label_site_nb<1>(a, st) : launch_label_site_nb<4>(a, st);
}

// The start of an AIS run with a label block, one wave per chain (the twin of k_ais_start).
//   draw: pixels v[row][c] = [u(row, c) < sigmoid(b_A[c])], c < n_pix; the class y from softmax(b_A[n_pix:]) by the label site's
//         recipe (max, exp, sum in class order, divide, running sum) with u(row, n_pix); the block becomes one-hot.
//   else: v is read; y = the first unit of the block above 1/2 (else C - 1).
//   vpart[row] = sum_{c < n_pix} (b_v - b_A)[c] v[row][c] + (b_v - b_A)[n_pix + y]: lane l adds pixels l, l + 64, ... in order, an
//   xor tree joins the lanes, the label term comes last.  logw[row] = 0 where logw is given.
__global__ __launch_bounds__(256) void k_ais_start_labels(float* __restrict__ v, int ldv, const float* __restrict__ b_v,
                                                          const float* __restrict__ base_bias, float* __restrict__ vpart,
                                                          double* __restrict__ logw, int rows, int n_pix, int C, int draw, RngArgs rng) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const uint64_t grow = rng.row0 + (uint64_t)row;
    const int word = (int)(grow & 3);
    float* vr = v + (size_t)row * ldv;
    float t = 0.f;
    for (int c = lane; c < n_pix; c += 64) {
        const float ba = base_bias[c];
        float x;
        if (draw) {
            uint32_t w[4];
            philox4x32_10((uint32_t)c, (uint32_t)(grow >> 2), rng.stream_id, rng.step, rng.seed_lo, rng.seed_hi, w);
            const uint32_t wr = word == 0 ? w[0] : (word == 1 ? w[1] : (word == 2 ? w[2] : w[3]));
            x = (u32_to_unit(wr) < sigmoidf_fast(ba)) ? 1.0f : 0.0f;
            vr[c] = x;
        } else {
            x = vr[c];
        }
        t += (b_v[c] - ba) * x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (lane == 0) {
        const float* bl = base_bias + n_pix;
        int y = -1;
        if (draw) {
            float mx = bl[0];
            for (int c = 1; c < C; ++c) mx = fmaxf(mx, bl[c]);
            float s = 0.f;
            for (int c = 0; c < C; ++c) s += expf(bl[c] - mx);
            uint32_t w[4];
            philox4x32_10((uint32_t)n_pix, (uint32_t)(grow >> 2), rng.stream_id, rng.step, rng.seed_lo, rng.seed_hi, w);
            const float u = u32_to_unit(word == 0 ? w[0] : (word == 1 ? w[1] : (word == 2 ? w[2] : w[3])));
            float cum = 0.f;
            for (int c = 0; c < C; ++c) {
                cum += expf(bl[c] - mx) / s;
                if (y < 0 && u < cum) y = c;
            }
            if (y < 0) y = C - 1;
            for (int c = 0; c < C; ++c) vr[n_pix + c] = (c == y) ? 1.0f : 0.0f;
        } else {
            for (int c = 0; c < C; ++c)
                if (y < 0 && vr[n_pix + c] > 0.5f) y = c;
            if (y < 0) y = C - 1;
        }
        vpart[row] = t + (b_v[n_pix + y] - bl[y]);
        if (logw) logw[row] = 0.0;
    }
}

hipError_t launch_ais_start_labels(float* v, int ldv, const float* b_v, const float* base_bias, float* vpart, double* logw, int rows,
                                   int n_pix, int C, int draw, const RngArgs& rng, hipStream_t st) {
    if (rows <= 0 || n_pix < 1 || C < 2 || C > 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ais_start_labels, dim3((rows + 3) / 4), dim3(256), 0, st, v, ldv, b_v, base_bias, vpart, logw, rows, n_pix, C,
                       draw, rng);
    return hipGetLastError();
}

}  // namespace kurbm
