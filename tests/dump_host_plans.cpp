// dump_host_plans.cpp -- what the host planning layer (keras_unsupervised_amd/csrc/kurbm_plan.h) computes, as JSON on stdout:
// every split-K plan, every workspace layout (member offsets, leading dimensions, size) and the plane formats of the x3 step,
// over a grid of shapes, options and knob settings.  No GPU, no HIP: g++ -std=c++17 -I keras_unsupervised_amd/csrc.
// tests/test_host_plans.py builds it and compares the output, key for key, with tests/golden/host_plans.json.xz.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <utility>

#include "kurbm_plan.h"

using namespace kurbm;

namespace {

// Carvers are given this address as the workspace: a member's offset is its pointer minus it (nothing is ever dereferenced)
char* const BASE = reinterpret_cast<char*>(uintptr_t(1) << 30);
long long off(const void* p) { return p ? (long long)(reinterpret_cast<uintptr_t>(p) - reinterpret_cast<uintptr_t>(BASE)) : -1; }

bool g_first = true;
std::string g_prefix;
void rec_open(const char* what, const std::string& tag = "") {
    printf("%s\"%s|%s%s%s\":{", g_first ? "{\n" : ",\n", g_prefix.c_str(), what, tag.empty() ? "" : "|", tag.c_str());
    g_first = false;
}
bool g_field0 = true;
void field(const char* name, long long v) { printf("%s\"%s\":%lld", g_field0 ? "" : ",", name, v); g_field0 = false; }
void rec_close() { printf("}"); g_field0 = true; }
#define F(s, x) field(#x, (long long)(s).x)
#define P(s, x) field(#x, off((s).x))

std::string tag(std::initializer_list<std::pair<const char*, long long>> kv) {
    std::string t;
    for (auto& p : kv) { if (!t.empty()) t += ","; t += p.first; t += "="; t += std::to_string(p.second); }
    return t;
}

template <class Plan> void plan_fields(const Plan& pl) {
    F(pl, cfg); F(pl, gm); F(pl, gn); F(pl, nkt); F(pl, kt_total); F(pl, nsplit); F(pl, nsplit_bound); F(pl, kt_per_split); F(pl, ld_slab);
}
template <class Plan> void dump_plan(const char* what, const std::string& t, const Plan& pl) { rec_open(what, t); plan_fields(pl); rec_close(); }

const int MODES[2] = {KURBM_MODE_VISIBLE_BERNOULLI, KURBM_MODE_VISIBLE_GAUSSIAN};
const int VPIECES[3] = {1, 1 | KURBM_V_BINARY, 3};
const int ROW_RANGES[3][2] = {{0, 128}, {128, 256}, {640, 784}};   // of the statistics of 784 visible units (kurbm_x3_stats_rows)

void dump_stats(const PlanCtx* ctx, int pieces, int vp, int mode, int rows, int nv, int nh, int m_lo, int m_hi) {
    const auto st = plan_stats(ctx, pieces, vp, mode, rows, nv, nh, m_lo, m_hi);
    const std::string t = tag({{"pieces", pieces}, {"vp", vp}, {"mode", mode}, {"lo", m_lo}, {"hi", m_hi}});
    rec_open("stats", t); F(st, nseg); F(st, slab_stride); rec_close();
    dump_plan("stats.pl", t, st.pl);
    dump_plan("stats.pos", t, st.sps.pos);
    dump_plan("stats.neg", t, st.sps.neg);
}

void dump_shape(const PlanCtx* ctx, int rows, int nv, int nh) {
    const int ldv_wide = (nv + 3) / 4 * 4 + 8;
    dump_plan("plan_outer", "", plan_outer(ctx, rows, nv, nh));
    for (int ldv : {0, ldv_wide}) {
        const auto w = carve_f32(ctx, BASE, rows, nv, nh, ldv);
        rec_open("carve_f32", tag({{"ldv", ldv}}));
        P(w, h_pos); P(w, h_neg); P(w, h_tmp); P(w, v_neg); P(w, part_h); P(w, part_v); P(w, slab); P(w, small_t);
        F(w, ldh); F(w, ldv); F(w, ld_part_h); F(w, ld_part_v); F(w, max_row_tiles); F(w, slab_stride); F(w, bytes);
        field("bytes_null", (long long)carve_f32(ctx, nullptr, rows, nv, nh, ldv).bytes);
        rec_close();
    }
    {
        const auto w = carve_ais(BASE, rows, nv, nh);
        rec_open("carve_ais");
        P(w, v); P(w, h); P(w, sppart); P(w, vpart); F(w, ldv); F(w, ldh); F(w, ld_part); F(w, ng_h); F(w, ng_v); F(w, bytes);
        field("bytes_null", (long long)carve_ais(nullptr, rows, nv, nh).bytes);
        rec_close();
    }
    {
        const auto w = carve_class(BASE, rows, nh);
        rec_open("carve_class"); P(w, a); F(w, lda); F(w, bytes); field("bytes_null", (long long)carve_class(nullptr, rows, nh).bytes); rec_close();
    }
    for (int C : {2, 10, 64}) {
        if (C >= nv) continue;
        dump_plan("plan_outer_one", tag({{"C", C}}), plan_outer_one(ctx, rows, nv - C, nh));
        for (int ldv : {0, ldv_wide}) {
            const auto w = carve_disc(ctx, BASE, rows, nv, nh, C, ldv);
            rec_open("carve_disc", tag({{"C", C}, {"ldv", ldv}}));
            P(w, a); P(w, logits); P(w, prob); P(w, g); P(w, nll); P(w, part); P(w, part_d); P(w, slab); P(w, delta); P(w, gen); P(w, cd);
            F(w, ldh); F(w, ldl); F(w, ld_part); F(w, ntiles); F(w, slab_stride); F(w, cd_bytes); F(w, bytes);
            field("bytes_null", (long long)carve_disc(ctx, nullptr, rows, nv, nh, C, ldv).bytes);
            rec_close();
        }
    }
    for (int pieces : {1, 3}) {
        const auto m = carve_mirror(ctx, BASE, nv, nh, pieces);
        rec_open("carve_mirror", tag({{"pieces", pieces}}));
        P(m, Wb); P(m, Wtb); F(m, Kh); F(m, Kv); F(m, ldW); F(m, ldWt); F(m, pieces); F(m, planeW); F(m, planeWt); F(m, bytes);
        field("bytes_null", (long long)carve_mirror(ctx, nullptr, nv, nh, pieces).bytes);
        rec_close();
    }
    for (int pieces : {1, 3})
        for (int vp : {1, 3}) {
            if (pieces == 1 && vp == 3) continue;
            const auto w = carve_bf16(ctx, BASE, rows, nv, nh, pieces, vp);
            rec_open("carve_bf16", tag({{"pieces", pieces}, {"vp", vp}}));
            P(w, vb); P(w, vbT); P(w, hb); P(w, hbT); P(w, v2b); P(w, v2bT); P(w, h2b); P(w, hnT); P(w, cb);
            P(w, part_h); P(w, part_v); P(w, slab); P(w, tmp32); P(w, rowpart);
            F(w, Kv); F(w, Kh); F(w, Kb); F(w, Lv); F(w, Lh); F(w, Lb); F(w, ldh32); F(w, ldv32); F(w, max_row_tiles);
            F(w, planeV); F(w, planeVT); F(w, planeHT); F(w, slab_stride); F(w, bytes);
            field("bytes_null", (long long)carve_bf16(ctx, nullptr, rows, nv, nh, pieces, vp).bytes);
            rec_close();
        }
    for (int vp : {1, 3}) {
        const auto v = carve_vplanes(ctx, BASE, rows, nv, vp);
        rec_open("carve_vplanes", tag({{"vp", vp}}));
        P(v, vb); P(v, vbT); P(v, part_v); F(v, bytes); field("bytes_null", (long long)carve_vplanes(ctx, nullptr, rows, nv, vp).bytes);
        rec_close();
        const auto f = carve_fe_x3(ctx, BASE, rows, nv, nh, vp);
        rec_open("carve_fe_x3", tag({{"vp", vp}}));
        P(f, Ab); P(f, rowpart); F(f, Lp); F(f, Kb); F(f, plane); F(f, grid_m); F(f, grid_n); F(f, ld_rowpart); F(f, bytes);
        field("bytes_null", (long long)carve_fe_x3(ctx, nullptr, rows, nv, nh, vp).bytes);
        rec_close();
    }
    for (int vp : VPIECES)
        for (int mode : MODES) {
            for (int clamp : {0, 1}) {
                const auto w = carve_gibbs(ctx, BASE, rows, nv, nh, vp, mode, clamp != 0);
                rec_open("carve_gibbs", tag({{"vp", vp}, {"mode", mode}, {"clamp", clamp}}));
                P(w, v0); P(w, vc); P(w, hb); P(w, maskp); F(w, Kv); F(w, Kh); F(w, Kb); F(w, Lv); F(w, Lh); F(w, sp); F(w, cp);
                F(w, sbytes); F(w, cbytes); F(w, hbytes); F(w, planeV); F(w, bytes);
                field("bytes_null", (long long)carve_gibbs(ctx, nullptr, rows, nv, nh, vp, mode, clamp != 0).bytes);
                rec_close();
            }
            dump_stats(ctx, 3, vp, mode, rows, nv, nh, 0, nv);
            if (nv == 784)
                for (auto& r : ROW_RANGES) dump_stats(ctx, 3, vp, mode, rows, nv, nh, r[0], r[1]);
        }
    for (int mode : MODES) dump_stats(ctx, 1, 1, mode, rows, nv, nh, 0, nv);
}

// the nine format flags of the x3 step and what kurbm_x3_dump_plane decodes each of its five planes as
void dump_formats(const PlanCtx* ctx, int nv) {
    const int rows = 100, nh = 260;
    for (int vp : VPIECES)
        for (int mode : MODES) {
            const PlaneFormats pf = plane_formats(ctx, 3, vp, mode, nv);
            const std::string t = tag({{"nv", nv}, {"vp", vp}, {"mode", mode}});
            rec_open("formats", t);
            F(pf, f8pos); F(pf, hbytes); F(pf, vbytes); F(pf, nbytes); F(pf, tbytes); F(pf, split_stats); F(pf, tbytes_n); F(pf, vneg_tr);
            F(pf, vn_pieces);
            rec_close();
            for (int which : {KURBM_PLANE_H_POS, KURBM_PLANE_H_POS_T, KURBM_PLANE_V_NEG, KURBM_PLANE_V_NEG_T, KURBM_PLANE_H_NEG_T}) {
                const PlaneView v = plane_view(ctx, BASE, which, rows, nv, nh, vp, mode);
                rec_open("view", t + ",which=" + std::to_string(which));
                P(v, src); F(v, units); F(v, fmt); F(v, ld); F(v, pieces); F(v, transposed); F(v, plane); field("sign", (long long)v.sign);
                rec_close();
            }
        }
}

const int ROWS[] = {1, 4, 31, 32, 33, 64, 100, 127, 128, 129, 512, 513, 4096};
const int SHAPES[][2] = {{1, 1}, {16, 8}, {128, 128}, {129, 64}, {130, 260}, {784, 1024}, {794, 1024}, {1024, 784}, {4096, 4096}};

}  // namespace

int main() {
    // default knobs: shapes x row counts, thinned to every second pair at 256 CUs and every fourth at 32 (the fixture stays small);
    // every shape and every row count still meets several of the other axis, under both CU counts
    for (int ncu : {256, 32}) {
        PlanCtx ctx;
        plan_ctx_init(&ctx, ncu);
        int i = 0;
        for (auto& s : SHAPES) {
            int j = 0;
            for (int rows : ROWS) {
                if ((i + j) % (ncu == 256 ? 2 : 4) == 0 || (ncu == 256 && rows == 128)) {   // (128 rows: one whole tile of the batch)
                    g_prefix = "ncu=" + std::to_string(ncu) + "|default|r=" + std::to_string(rows) + ",v=" + std::to_string(s[0]) + ",h=" + std::to_string(s[1]);
                    dump_shape(&ctx, rows, s[0], s[1]);
                }
                ++j;
            }
            ++i;
        }
        for (int nv : {128, 129, 784}) {
            g_prefix = "ncu=" + std::to_string(ncu) + "|default";
            dump_formats(&ctx, nv);
        }
    }
    // one knob off its default at a time, three shapes each
    const struct { const char* name; int value; } SETTINGS[] = {
        {"KURBM_SPLIT", 2}, {"KURBM_CFG_OUTER", 1}, {"KURBM_BF16_SPLIT", 3}, {"KURBM_X3_SPLIT_STATS", 0}, {"KURBM_X3_STATS_TALL", 0},
        {"KURBM_X3_BYTES", 0}, {"KURBM_LDPAD", 8}};
    const int KNOB_SHAPES[][3] = {{100, 130, 260}, {128, 784, 1024}, {513, 1024, 784}};
    for (auto& k : SETTINGS) {
        PlanCtx ctx;
        plan_ctx_init(&ctx, 256);
        if (!plan_ctx_set(&ctx, k.name, k.value)) { fprintf(stderr, "unknown knob %s\n", k.name); return 1; }
        const std::string head = std::string("ncu=256|") + k.name + "=" + std::to_string(k.value);
        for (auto& s : KNOB_SHAPES) {
            g_prefix = head + "|r=" + std::to_string(s[0]) + ",v=" + std::to_string(s[1]) + ",h=" + std::to_string(s[2]);
            dump_shape(&ctx, s[0], s[1], s[2]);
        }
        for (int nv : {128, 129, 784}) {
            g_prefix = head;
            dump_formats(&ctx, nv);
        }
    }
    printf("\n}\n");
    return 0;
}
