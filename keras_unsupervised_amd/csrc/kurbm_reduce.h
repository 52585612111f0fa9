// kurbm_reduce.h -- the bodies of the launches that reduce the statistics and apply the update, as templates on the MOM flag
// (momentum / weight decay: kurbm_kernels.h, MomArgs).  The ordinary kernels are instantiated where they always were
// (k_reduce_apply: kurbm_kernels.hip; k_reduce_apply_split, _peer: kurbm_bf16.hip); the MOM kernels live in a file of their own,
// kurbm_mom.hip, so that the code objects of the other files -- what a run without momentum loads -- hold exactly the kernels
// they held before.
#pragma once
#include "kurbm_kernels.h"
#include "kurbm_device.h"

namespace kurbm {

constexpr int CVT = 64;   // columns of a conversion / reduce tile (kurbm_bf16.hip)

// ---- slab reduction + parameter update + weight-piece mirror (kurbm_bf16.hip has the description) ----
template <int TR, bool PEER, bool MOM>
__device__ __forceinline__ void reduce_apply_split_body(ReduceArgs& a, int tiles_x, int tiles, int nbias, const PeerSrc& ps, const MomArgs& mo) {
    static_assert(!(PEER && MOM), "the peer exchange's apply has no momentum");
    __shared__ __attribute__((aligned(16))) float tile[TR][CVT + 1];
    __shared__ int peer_ok;
    const int t = threadIdx.x;
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    if constexpr (PEER) {
        if (blockIdx.x == 0) {
            if (t == 0) peer_ok = 1;
            __syncthreads();
            if (t < ps.nranks && !wait_flag_ge(ps.summed[t], ps.epoch, ps.timeout_ticks)) peer_ok = 0;
            __syncthreads();
            if (!peer_ok) {
                if (t == 0) __hip_atomic_fetch_or(ps.status, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
        }
    }
    // the first nbias blocks: bias column sums (kurbm_kernels.h); then the tiles of W
    if ((int)blockIdx.x < nbias) {
        bias_colsum_wave_t<MOM>(a, mo, blockIdx.x * 4 + (t >> 6), t & 63);
        return;
    }
    const int tb = (int)blockIdx.x - nbias;
    if (tb < tiles) {
        const int by = tb / tiles_x, bx = tb - by * tiles_x;
        if constexpr (PEER) {
            // the band of this tile's rows (band_rows is a multiple of TR; tiles past the matrix only write mirror padding)
            int q = (by * TR) / ps.band_rows;
            if (q >= ps.nranks) q = ps.nranks - 1;
            if (t == 0) peer_ok = (by * TR >= a.n_vis || wait_flag_ge(ps.summed[q], ps.epoch, ps.timeout_ticks)) ? 1 : 0;
            __syncthreads();
            if (!peer_ok) {
                if (t == 0) __hip_atomic_fetch_or(ps.status, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            a.slab = ps.sum[q];      // (nslab = 1, ld_slab = n_hid: the packed layout)
        }
        const int q4 = (t & 15) * 4, rq = t >> 4;
        const int c = bx * CVT + q4;
        auto store3 = [&](uint16_t* dst, size_t plane, float v0, float v1, float v2, float v3) {
            float v[4] = {v0, v1, v2, v3};
            for (int j = 0; j < a.pieces; ++j) {
                u32x2 pk;
                pk.x = pack_bf16x2(v[0], v[1]); pk.y = pack_bf16x2(v[2], v[3]);
                *reinterpret_cast<u32x2*>(dst + j * plane) = pk;
                if (j + 1 < a.pieces) {
                    v[0] -= bf16_bits_to_f32(pk.x & 0xFFFFu); v[1] -= bf16_bits_to_f32(pk.x >> 16);
                    v[2] -= bf16_bits_to_f32(pk.y & 0xFFFFu); v[3] -= bf16_bits_to_f32(pk.y >> 16);
                }
            }
        };
        // Every load of the thread's TR / 16 rows goes out before the first sum: the rows' weights and their first four slabs (this launch
        // is a burst of ~17 MB of loads that every CU must keep in flight: with the rows one after the other a wave held 5 x 16 bytes per
        // lane in flight, now TR / 16 times that).  The slabs are still added in slab order, row by row: the same bits as before.
        constexpr int NJ = TR / 16;
        f32x4 wv[NJ], sv[NJ][4];
        f32x4 vv[MOM ? NJ : 1];      // MOM: the rows' velocity groups travel with their weights (n_hid % 4 == 0: whole groups, aligned)
        bool live[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int r = by * TR + rq + 16 * j;
            live[j] = r < a.n_vis && c < a.n_hid;
            wv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int z = 0; z < 4; ++z) sv[j][z] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (MOM) {
                vv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (live[j]) vv[j] = *reinterpret_cast<const f32x4*>(mo.vel_w + (size_t)r * a.n_hid + c);
            }
            if (live[j]) {
                if (a.W) wv[j] = *reinterpret_cast<const f32x4*>(a.W + (size_t)r * a.ldw + c);           // ldw % 4 == 0
                if (a.slab) {
                    const float* sp = a.slab + (size_t)r * a.ld_slab + c;    // ld_slab % 4 == 0: the group stays inside the row
#pragma unroll
                    for (int z = 0; z < 4; ++z)
                        if (z < a.nslab) sv[j][z] = *reinterpret_cast<const f32x4*>(sp + (size_t)z * a.slab_stride);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int r = by * TR + rq + 16 * j;
            f32x4 w = {0.f, 0.f, 0.f, 0.f};
            if (live[j]) {
                f32x4 s = {0.f, 0.f, 0.f, 0.f};
                if (a.slab) {
                    const float* sp = a.slab + (size_t)r * a.ld_slab + c;
#pragma unroll
                    for (int z = 0; z < 4; ++z)
                        if (z < a.nslab) s += sv[j][z];
                    int zz = 4;
                    for (; zz + 4 <= a.nslab; zz += 4) {
                        const f32x4 v0 = *reinterpret_cast<const f32x4*>(sp + (size_t)(zz + 0) * a.slab_stride);
                        const f32x4 v1 = *reinterpret_cast<const f32x4*>(sp + (size_t)(zz + 1) * a.slab_stride);
                        const f32x4 v2 = *reinterpret_cast<const f32x4*>(sp + (size_t)(zz + 2) * a.slab_stride);
                        const f32x4 v3 = *reinterpret_cast<const f32x4*>(sp + (size_t)(zz + 3) * a.slab_stride);
                        s += v0; s += v1; s += v2; s += v3;
                    }
                    for (; zz < a.nslab; ++zz) s += *reinterpret_cast<const f32x4*>(sp + (size_t)zz * a.slab_stride);
                }
                if (a.W) {
                    float* wp = a.W + (size_t)r * a.ldw + c;
                    w = wv[j];
                    if constexpr (MOM) {
                        const f32x4 vel = vv[j] * mo.mu + (s - w * mo.decay) * a.lr;
                        *reinterpret_cast<f32x4*>(mo.vel_w + (size_t)r * a.n_hid + c) = vel;
                        w = w + vel;
                    } else if (a.slab) w = w + s * a.lr;
                    // the tail group of a row (n_hid % 4 != 0): W's padding columns go back as they were loaded (include/kurbm.h: output
                    // padding is left untouched -- it may be NaN), and enter the bf16 pieces below as zeros
                    f32x4 wst = w;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e >= a.n_hid) { wst[e] = wv[j][e]; w[e] = 0.f; }
                    if (a.slab) *reinterpret_cast<f32x4*>(wp) = wst;
                }
                if (a.delta_w) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < a.n_hid) a.delta_w[(size_t)r * a.n_hid + c + e] = s[e];
                }
            }
            tile[rq + 16 * j][q4 + 0] = w.x; tile[rq + 16 * j][q4 + 1] = w.y;
            tile[rq + 16 * j][q4 + 2] = w.z; tile[rq + 16 * j][q4 + 3] = w.w;
            if (a.Wb && r < a.n_vis && c < a.ldWb) store3(a.Wb + (size_t)r * a.ldWb + c, a.planeWb, w.x, w.y, w.z, w.w);
        }
        __syncthreads();
        if (a.Wtb) {
            // TR / 4 lanes x 4 rows down a column of the tile (a run of 2 TR bytes per column), 1024 / TR columns per pass
            constexpr int LPC = TR / 4, CPP = 256 / LPC;
            const int rr4 = (t % LPC) * 4, cq = t / LPC;
            const int rr = by * TR + rr4;
#pragma unroll
            for (int j = 0; j < CVT / CPP; ++j) {
                const int cl = cq + CPP * j, cc = bx * CVT + cl;
                if (cc < a.n_hid && rr < (a.wtb_k_ext ? a.wtb_k_ext : a.ldWtb))
                    store3(a.Wtb + (size_t)cc * a.ldWtb + rr, a.planeWtb, tile[rr4 + 0][cl], tile[rr4 + 1][cl], tile[rr4 + 2][cl],
                           tile[rr4 + 3][cl]);
            }
        }
        return;
    }
}

// ---- slab reduction (+ parameter update) on the fp32 path (kurbm_kernels.hip has the description) ----
__device__ __forceinline__ void mom_w4(float* wp, float* vp, const f32x4 s, float lr, const MomArgs& mo, bool vel_aligned) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(wp);
    f32x4 v;
    if (vel_aligned) v = *reinterpret_cast<const f32x4*>(vp);
    else v = f32x4{vp[0], vp[1], vp[2], vp[3]};
    v = v * mo.mu + (s - w * mo.decay) * lr;
    if (vel_aligned) *reinterpret_cast<f32x4*>(vp) = v;
    else { vp[0] = v.x; vp[1] = v.y; vp[2] = v.z; vp[3] = v.w; }
    *reinterpret_cast<f32x4*>(wp) = w + v;
}
__device__ __forceinline__ void mom_w1(float* wp, float* vp, float s, float lr, const MomArgs& mo) {
    const float w = *wp, v = mo.mu * *vp + lr * (s - mo.decay * w);
    *vp = v;
    *wp = w + v;
}
template <bool MOM>
__device__ __forceinline__ void reduce_apply_body(const ReduceArgs a, const MomArgs mo, const int nbias, const int nbias8) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < nbias8) {
        if ((int)blockIdx.x < nbias) bias_colsum_wave_t<MOM>(a, mo, blockIdx.x * 4 + (tid >> 6), tid & 63);
        return;
    }
    const int blk = (int)blockIdx.x - nbias8;
    if (blk < a.nblk_w) {
        if (a.tile_bm > 0) {
            // tile order: the same XCD remap as the GEMM, then (tile, part of the tile)
            const int nwg = a.nblk_w;
            int bid = blk;
            const int xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
            bid = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
            const int tile = bid / a.parts, part = bid - tile * a.parts;
            const int bm = a.m_fastest ? tile % a.grid_m : tile / a.grid_n;
            const int bn = a.m_fastest ? tile / a.grid_m : tile - bm * a.grid_n;
            const int g4 = a.tile_bn / 4;
            const int rows_pp = (a.tile_bm + a.parts - 1) / a.parts;
            // one block = rows_pp x tile_bn floats; lanes walk the float4 groups of a row
            for (int e = tid; e < rows_pp * g4; e += 256) {
                const int r = part * rows_pp + e / g4;
                const int ii = bm * a.tile_bm + r, jj = bn * a.tile_bn + 4 * (e % g4);
                if (r >= a.tile_bm || ii >= a.n_vis || jj >= a.n_hid) continue;
                const float* sp = a.slab + (size_t)ii * a.ld_slab + jj;
                f32x4 s = {0.f, 0.f, 0.f, 0.f};
                int zz = 0;
                for (; zz + 4 <= a.nslab; zz += 4) {
                    const f32x4 v0 = *reinterpret_cast<const f32x4*>(sp + (size_t)(zz + 0) * a.slab_stride);
                    const f32x4 v1 = *reinterpret_cast<const f32x4*>(sp + (size_t)(zz + 1) * a.slab_stride);
                    const f32x4 v2 = *reinterpret_cast<const f32x4*>(sp + (size_t)(zz + 2) * a.slab_stride);
                    const f32x4 v3 = *reinterpret_cast<const f32x4*>(sp + (size_t)(zz + 3) * a.slab_stride);
                    s += v0; s += v1; s += v2; s += v3;
                }
                for (; zz < a.nslab; ++zz) s += *reinterpret_cast<const f32x4*>(sp + (size_t)zz * a.slab_stride);
                if (jj + 3 < a.n_hid) {
                    if (a.W) {
                        if constexpr (MOM) {
                            mom_w4(a.W + (size_t)ii * a.ldw + jj, mo.vel_w + (size_t)ii * a.n_hid + jj, s, a.lr, mo, (a.n_hid & 3) == 0);
                        } else {
                            f32x4* w = reinterpret_cast<f32x4*>(a.W + (size_t)ii * a.ldw + jj);
                            *w = *w + s * a.lr;
                        }
                    }
                    if (a.delta_w) {
                        float* d = a.delta_w + (size_t)ii * a.n_hid + jj;
                        if ((a.n_hid & 3) == 0) *reinterpret_cast<f32x4*>(d) = s;
                        else { d[0] = s.x; d[1] = s.y; d[2] = s.z; d[3] = s.w; }
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (jj + u < a.n_hid) {
                            if (a.delta_w) a.delta_w[(size_t)ii * a.n_hid + jj + u] = s[u];
                            if constexpr (MOM) {
                                if (a.W) mom_w1(a.W + (size_t)ii * a.ldw + jj + u, mo.vel_w + (size_t)ii * a.n_hid + jj + u, s[u], a.lr, mo);
                            } else if (a.W) a.W[(size_t)ii * a.ldw + jj + u] += a.lr * s[u];
                        }
                }
            }
            return;
        }
    }
    if (blk < a.nblk_w) {   // row order (no tile geometry given)
        const int groups = a.ld_slab / 4;  // float4 groups per row
        const long long q = (long long)blk * 256 + tid;
        if (q >= (long long)a.n_vis * groups) return;
        const int i = (int)(q / groups), j0 = (int)(q - (long long)i * groups) * 4;
        // slabs are summed in index order (bit-reproducible); four loads in flight per lane
        const float* sp = a.slab + (size_t)i * a.ld_slab + j0;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        int zz = 0;
        for (; zz + 4 <= a.nslab; zz += 4) {
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(sp + (size_t)(zz + 0) * a.slab_stride);
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(sp + (size_t)(zz + 1) * a.slab_stride);
            const f32x4 v2 = *reinterpret_cast<const f32x4*>(sp + (size_t)(zz + 2) * a.slab_stride);
            const f32x4 v3 = *reinterpret_cast<const f32x4*>(sp + (size_t)(zz + 3) * a.slab_stride);
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; zz < a.nslab; ++zz) s += *reinterpret_cast<const f32x4*>(sp + (size_t)zz * a.slab_stride);
        if (j0 + 3 < a.n_hid) {   // whole 16-B group inside the matrix: vector read-modify-write
            if (a.W) {
                if constexpr (MOM) {
                    mom_w4(a.W + (size_t)i * a.ldw + j0, mo.vel_w + (size_t)i * a.n_hid + j0, s, a.lr, mo, (a.n_hid & 3) == 0);
                } else {
                    f32x4* w = reinterpret_cast<f32x4*>(a.W + (size_t)i * a.ldw + j0);
                    *w = *w + s * a.lr;
                }
            }
            if (a.delta_w) {
                float* d = a.delta_w + (size_t)i * a.n_hid + j0;
                if ((a.n_hid & 3) == 0) *reinterpret_cast<f32x4*>(d) = s;
                else { d[0] = s.x; d[1] = s.y; d[2] = s.z; d[3] = s.w; }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = j0 + e;
                if (j < a.n_hid) {
                    if (a.delta_w) a.delta_w[(size_t)i * a.n_hid + j] = s[e];
                    if constexpr (MOM) {
                        if (a.W) mom_w1(a.W + (size_t)i * a.ldw + j, mo.vel_w + (size_t)i * a.n_hid + j, s[e], a.lr, mo);
                    } else if (a.W) a.W[(size_t)i * a.ldw + j] += a.lr * s[e];
                }
            }
        }
        return;
    }
}

}  // namespace kurbm
