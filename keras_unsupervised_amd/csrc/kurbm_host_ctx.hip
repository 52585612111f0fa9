// kurbm_host_ctx.hip -- the context, the error record, the knobs and the small utilities of the C ABI (include/kurbm.h).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "kurbm_host.h"

using namespace kurbm;

static thread_local std::string g_err;

namespace kurbm {
unsigned* ctx_status_word(kurbm_ctx* ctx) { return ctx ? ctx->status : nullptr; }
int fail_msg(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace kurbm

extern "C" {

int kurbm_abi_version(void) { return KURBM_ABI_VERSION; }

const char* kurbm_last_error(void) { return g_err.c_str(); }

int kurbm_ctx_create(int device, kurbm_ctx** out) {
    if (!out) return fail_msg(KURBM_ERR_ARG, "out is null");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail_msg(KURBM_ERR_ARG, "device %d out of range (%d visible)", device, n);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail_msg(KURBM_ERR_UNSUPPORTED, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    kurbm_ctx* c = new kurbm_ctx;
    c->device = device;
    c->plan.ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    for (int i = 0; i < KN_COUNT; ++i) {
        const char* v = getenv(KNOBS[i].env);
        c->plan.knob[i] = (v && *v) ? atoi(v) : KNOBS[i].dflt;
    }
    c->status = nullptr;
    {
        const int ncu = c->plan.ncu;
        int prev = 0;
        (void)hipGetDevice(&prev);
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->status), STATUS_BYTES);
        if (e == hipSuccess) e = hipMemset(c->status, 0, STATUS_BYTES);
        // where do the workgroups of a grid run?  (the XCD-local schedule of the one-launch small step stands on the answer)
        c->xcc_round_robin = 0; c->xcc_map = 0;
        if (e == hipSuccess && ncu >= 8 && ncu <= 1024) {
            unsigned* probe = nullptr;
            unsigned host[1024];
            if (hipMalloc(reinterpret_cast<void**>(&probe), sizeof(unsigned) * ncu) == hipSuccess) {
                if (launch_xcc_probe(probe, ncu, nullptr) == hipSuccess &&
                    hipMemcpy(host, probe, sizeof(unsigned) * ncu, hipMemcpyDeviceToHost) == hipSuccess) {
                    // the model the schedule stands on: eight XCDs, and on each of them exactly one workgroup of every octet
                    // (workgroup b: octet b / 8) -- consecutive workgroups go to consecutive XCDs, from wherever the dispatcher stood
                    bool rr = (ncu % 8) == 0;
                    unsigned seen[8][32];
                    memset(seen, 0, sizeof seen);
                    for (int b = 0; rr && b < ncu; ++b) {
                        const unsigned x = host[b];
                        if (x > 7u || (seen[x][(b >> 3) >> 5] >> ((b >> 3) & 31)) & 1u) rr = false;
                        else seen[x][(b >> 3) >> 5] |= 1u << ((b >> 3) & 31);
                    }
                    if (rr) {
                        c->xcc_round_robin = 1;
                        for (int g = 0; g < 8; ++g) c->xcc_map |= (host[g] & 15u) << (4 * g);
                    }
                }
                (void)hipFree(probe);
            }
            (void)hipGetLastError();
        }
        (void)hipSetDevice(prev);
        if (e != hipSuccess) {
            if (c->status) (void)hipFree(c->status);
            delete c;
            return fail_msg(KURBM_ERR_HIP, "status word of the context: %s", hipGetErrorString(e));
        }
    }
    *out = c;
    return KURBM_OK;
}

int kurbm_ctx_status(kurbm_ctx* ctx, int* bits) {
    if (!ctx || !bits) return fail_msg(KURBM_ERR_ARG, "null argument");
    unsigned v = 0;
    HIP_TRY(hipMemcpy(&v, ctx->status, sizeof v, hipMemcpyDeviceToHost));      // (synchronises with the device)
    if (v) HIP_TRY(hipMemset(ctx->status, 0, STATUS_BYTES));      // (also re-arms the grid barrier of kurbm_cd_step_small)
    *bits = (int)v;
    return KURBM_OK;
}

int kurbm_ctx_set_option(kurbm_ctx* ctx, const char* name, int value) {
    if (!ctx || !name) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (!plan_ctx_set(&ctx->plan, name, value)) return fail_msg(KURBM_ERR_ARG, "unknown option %s", name);
    return KURBM_OK;
}

void kurbm_ctx_destroy(kurbm_ctx* ctx) {
    if (!ctx) return;
    if (ctx->status) (void)hipFree(ctx->status);
    delete ctx;
}

int kurbm_philox_uniform(kurbm_ctx* ctx, float* out, int rows, int cols, int ld, const kurbm_rng* rng,
                         kurbm_stream_t stream) {
    if (!ctx || !out || !rng) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (rows <= 0 || cols <= 0 || ld < cols) return fail_msg(KURBM_ERR_ARG, "bad shape");
    if (rng->row0 & 3) return fail_msg(KURBM_ERR_ARG, "rng.row0 must be a multiple of 4");
    HIP_TRY(launch_philox_uniform(out, rows, cols, ld, make_rng(rng), static_cast<hipStream_t>(stream)));
    return KURBM_OK;
}

int kurbm_bf16_exact(kurbm_ctx* ctx, const float* x, int rows, int cols, int ld, int* flag, kurbm_stream_t stream) {
    if (!ctx || !flag) return fail_msg(KURBM_ERR_ARG, "null argument");
    if (rows <= 0 || cols <= 0 || bad_matrix(x, ld, cols)) return fail_msg(KURBM_ERR_ARG, "x: null, misaligned, ld %% 4 != 0 or ld < cols");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), st));
    HIP_TRY(launch_bf16_exact_check(x, rows, cols, ld, flag, st));
    return KURBM_OK;
}

#ifdef KURBM_SMALL_STAMPS
/* diagnostic build only: the eight phase stamps of the last kurbm_cd_step_small (100 MHz ticks) */
int kurbm_debug_small_stamps(kurbm_ctx* ctx, unsigned long long* out8) {
    HIP_TRY(hipMemcpy(out8, ctx->status + 40, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return KURBM_OK;
}
/* ... and the fine stamps of the h -> v phase (workgroup 0, its first pass) */
int kurbm_debug_small_fine_stamps(kurbm_ctx* ctx, unsigned long long* out8) {
    HIP_TRY(hipMemcpy(out8, ctx->status + 768, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return KURBM_OK;
}
#endif
#ifdef KURBM_STAMPS
/* diagnostic library only: not part of include/kurbm.h */
void kurbm_debug_set_stamp_buffer(void* p) { set_stamp_buffer(static_cast<unsigned long long*>(p)); }
void kurbm_debug_set_off(int mask) { set_debug_off(mask); }
#endif

}  // extern "C"
