// dqrm_host.hip — what every unit of libdqrm depends on, host code only (no kernel): the error
// path, the environment switches, and the validators the exports of several units share
// (declared in dqrm_internal.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <stdlib.h>

#include "../../include/dqrm.h"
#include "dqrm_internal.h"
#include "dqrm_device.h"

namespace {

using dqrm_internal::set_error;

// ------------------------------------------------------------------------------------
// error reporting (host)
// ------------------------------------------------------------------------------------
thread_local char g_last_error[512] = "";

}  // namespace

int dqrm_internal::set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
    va_end(ap);
    return code;
}

// ------------------------------------------------------------------------------------
// The environment switches (host): every DQRM_* variable libdqrm reads is read here and nowhere
// else; dqrm_internal.h documents each accessor (values, default, what it selects), and
// INTEGRATION.md lists them all. Read once per process, on first use, unless said otherwise.
// ------------------------------------------------------------------------------------
static bool env_is(const char* e, const char* value) { return e && !strcmp(e, value); }
static uint32_t env_u32(const char* e, uint32_t dflt) { return e ? (uint32_t)strtoul(e, nullptr, 10) : dflt; }

// Unset or anything else: the default, y ("write-through stores of once-written
// outputs": the hand-over buffers gained on the forced-collectives line only and moved no
// WRITE_SIZE, the wide tables' W rows did not gain and are not in the code).
uint32_t dqrm_internal::wt_stores(int dim) {
    static const uint32_t v = [] {
        const char* e = getenv("DQRM_WT_STORES");
        if (env_is(e, "0")) return 0u;
        if (env_is(e, "hand")) return WT_HAND;
        if (env_is(e, "all")) return WT_Y | WT_HAND;
        return WT_Y;
    }();
    return dim * (int)sizeof(float) >= 128 ? v : v & ~WT_Y;  // y rows of whole L2 lines only
}
int dqrm_internal::env_apply() {  // not cached here: apply_kernel_kind() holds the value
    const char* e = getenv("DQRM_APPLY");
    return env_is(e, "flat") ? DQRM_APPLY_FLAT : env_is(e, "slot") ? DQRM_APPLY_SLOT
           : env_is(e, "ranges") ? DQRM_APPLY_RANGES : env_is(e, "merge") ? DQRM_APPLY_MERGE : DQRM_APPLY_AUTO;
}
int dqrm_internal::env_finalize() {
    static const int v = [] {
        const char* e = getenv("DQRM_FINALIZE");
        return env_is(e, "launch") ? 1 : env_is(e, "inline") ? 2 : 0;
    }();
    return v;
}
bool dqrm_internal::env_fin_flagged() {
    static const bool off = env_is(getenv("DQRM_FIN_FLAGGED"), "0");
    return !off;
}
bool dqrm_internal::env_fused_fwd() {
    static const bool off = env_is(getenv("DQRM_FUSED_FWD"), "0");
    return !off;
}
bool dqrm_internal::env_fin_fwd() {
    static const bool off = env_is(getenv("DQRM_FIN_FWD"), "0");
    return !off;
}
bool dqrm_internal::env_local_fused() {
    static const bool off = env_is(getenv("DQRM_LOCAL_FUSED"), "0");
    return !off;
}
bool dqrm_internal::env_qpack_legacy() {
    static const bool v = env_is(getenv("DQRM_QPACK"), "legacy");
    return v;
}
int64_t dqrm_internal::env_merge_keys() {
    static const int64_t v = [] {
        const char* e = getenv("DQRM_MERGE_KEYS");
        const long k = e ? atol(e) : 256;
        return (int64_t)(k > 0 ? k : 256);
    }();
    return v;
}
int dqrm_internal::env_merge_diag() {
    static const int v = [] {
        const char* e = getenv("DQRM_MERGE_DIAG");
        return e ? atoi(e) : 0;
    }();
    return v;
}
int dqrm_internal::env_flat_dual() {  // read on every call: tests switch it inside one process
    const char* e = getenv("DQRM_FLAT_DUAL");
    return e ? atoi(e) : -1;
}
uint32_t dqrm_internal::env_gate_spin() {
    static const uint32_t v = env_u32(getenv("DQRM_GATE_SPIN"), 1u << 20);
    return v;
}
uint32_t dqrm_internal::env_stall_spin() {
    static const uint32_t v = env_u32(getenv("DQRM_STALL_SPIN"), 1u << 20);
    return v;
}
bool dqrm_internal::env_subslots() {
    static const bool off = env_is(getenv("DQRM_SUBSLOTS"), "0");
    return !off;
}
bool dqrm_internal::env_subslot_small_first() {
    static const bool v = env_is(getenv("DQRM_SUBSLOT_ORDER"), "small");
    return v;
}
bool dqrm_internal::env_table_groups_critical() {
    static const bool v = env_is(getenv("DQRM_TABLE_GROUPS"), "critical");
    return v;
}

// ------------------------------------------------------------------------------------
// The checks several exports share; `who` is the export name the text reports.
// ------------------------------------------------------------------------------------
int dqrm_internal::check_set(const dqrm_table_set* s) {
    if (!s) return set_error(DQRM_E_INVALID, "dqrm: null table set");
    if (s->num_tables <= 0 || s->num_tables > kMaxTables)
        return set_error(DQRM_E_INVALID, "dqrm: num_tables out of range (%d)", s->num_tables);
    const int D = s->dim;
    if (D < 4 || D > 256 || (D & 3) || ((D / 4) & (D / 4 - 1)))
        return set_error(DQRM_E_INVALID, "dqrm: dim must be 4*2^k <= 256 (got %d)", D);
    if (!s->W || !s->rowmax || !s->blkmax || !s->sblkmax || !s->tmax || !s->scale || !s->pscale ||
        !s->meta || !s->err || !s->tflags || !s->sdirty || !s->bdirty || !s->sync)
        return set_error(DQRM_E_INVALID, "dqrm: null state pointer");
    if (((uintptr_t)s->W) & 15)
        return set_error(DQRM_E_INVALID, "dqrm: W must be 16-byte aligned");
    return DQRM_OK;
}

int dqrm_internal::check_batch(const dqrm_batch* batch, const char* who) {
    if (!batch || !batch->idx || !batch->off || !batch->idx_base)
        return set_error(DQRM_E_INVALID, "%s: null batch pointer", who);
    if (batch->num_bags > 0xFFFFFFFFll)
        return set_error(DQRM_E_CAPACITY, "%s: more than 2^32 bags", who);
    return DQRM_OK;
}

int dqrm_internal::check_dy(const float* dy, int64_t dy_stride_t, int64_t dy_stride_b, const char* who) {
    if (!dy || (((uintptr_t)dy) & 15) || (dy_stride_t & 3) || (dy_stride_b & 3))
        return set_error(DQRM_E_INVALID, "%s: dy must be 16-B aligned with strides %% 4 == 0", who);
    return DQRM_OK;
}

int dqrm_internal::check_repack(const dqrm_table_set* set, int repack_bits, const char* who) {
    if (repack_bits && (repack_bits != 4 || !set->packed))
        return set_error(DQRM_E_INVALID, "%s: repack needs packed rows and bits == 4 (got %d)", who, repack_bits);
    return DQRM_OK;
}

int dqrm_internal::check_slot_ws(const int64_t* ws_cap_base, const int32_t* ws_rows, const float* ws_vals,
                                 const int32_t* ws_ucount, const float* ws_absmax, const char* who, bool rest_ok) {
    if (!ws_cap_base || !ws_rows || !ws_vals || !ws_ucount || !ws_absmax || !rest_ok || (((uintptr_t)ws_vals) & 15))
        return set_error(DQRM_E_INVALID, "%s: null/unaligned workspace", who);
    return DQRM_OK;
}

int dqrm_internal::grid_for(int64_t work_items, int threads, int max_blocks) {
    int64_t b = (work_items + threads - 1) / threads;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (int)b;
}

extern "C" {

const char* dqrm_last_error(void) { return g_last_error; }

int dqrm_abi_version(void) { return DQRM_ABI_VERSION; }

int dqrm_read_errors(const dqrm_table_set* set, uint32_t* flags, int clear, void* stream) {
    if (!set || !set->err || !flags) return set_error(DQRM_E_INVALID, "%s: null pointer", "dqrm_read_errors");
    hipStream_t st = (hipStream_t)stream;
    DQRM_HIP_TRY(hipMemcpyAsync(flags, set->err, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    DQRM_HIP_TRY(hipStreamSynchronize(st));
    if (clear) DQRM_HIP_TRY(hipMemsetAsync(set->err, 0, sizeof(uint32_t), st));
    return DQRM_OK;
}

}  // extern "C"
