// dqrm_internal.h — what the translation units of libdqrm share on the host (not part of the
// C ABI; include/dqrm.h is): the error path, the environment switches and the validators
// (dqrm_host.hip's), the dimension dispatch, the validation one unit does for another, and the
// launch interface between units. A new unit includes this and defines no copy of any of it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dqrm.h"

namespace dqrm_internal {

#define DQRM_HIDDEN __attribute__((visibility("hidden")))

// The one error path: formats into the calling thread's dqrm_last_error() text and returns
// `code` (dqrm_host.hip).
DQRM_HIDDEN __attribute__((format(printf, 2, 3))) int set_error(int code, const char* fmt, ...);

#define DQRM_HIP_TRY(expr)                                                                                      \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess)                                                                                   \
            return dqrm_internal::set_error(DQRM_E_HIP, "HIP error: %s (%d)", hipGetErrorString(e_), (int)e_); \
    } while (0)
#define LAUNCH_CHECK() DQRM_HIP_TRY(hipGetLastError())

// Runs the statement with LPR = D / 4 (lanes per row, a float4 each) as a constant.
#define DISPATCH_LPR(D, ...)                                  \
    switch ((D) / 4) {                                        \
        case 1: { constexpr int LPR = 1; __VA_ARGS__; } break;  \
        case 2: { constexpr int LPR = 2; __VA_ARGS__; } break;  \
        case 4: { constexpr int LPR = 4; __VA_ARGS__; } break;  \
        case 8: { constexpr int LPR = 8; __VA_ARGS__; } break;  \
        case 16: { constexpr int LPR = 16; __VA_ARGS__; } break; \
        case 32: { constexpr int LPR = 32; __VA_ARGS__; } break; \
        case 64: { constexpr int LPR = 64; __VA_ARGS__; } break; \
        default: return dqrm_internal::set_error(DQRM_E_INVALID, "dqrm: unsupported dim %d", (int)(D)); \
    }

constexpr int kMaxTables = 256;  // tables of a dqrm_table_set or dqrm_rowwise_set

// ---- The validators several units' exports share (dqrm_host.hip); `who`: the export the text names.
// the table set: non-null, 1..kMaxTables tables, dim 4*2^k <= 256, every state pointer, W 16-B aligned
DQRM_HIDDEN int check_set(const dqrm_table_set* s);
// the batch: its three pointers, and at most 2^32 bags (DQRM_E_CAPACITY)
DQRM_HIDDEN int check_batch(const dqrm_batch* batch, const char* who);
// dy: non-null, 16-B aligned, strides % 4 == 0
DQRM_HIDDEN int check_dy(const float* dy, int64_t dy_stride_t, int64_t dy_stride_b, const char* who);
// repack_bits: 0, or 4 on a set with packed rows
DQRM_HIDDEN int check_repack(const dqrm_table_set* set, int repack_bits, const char* who);
// the coalesced-gradient slot workspace; rest_ok: what else the caller needs of it (s_avg, a total)
DQRM_HIDDEN int check_slot_ws(const int64_t* ws_cap_base, const int32_t* ws_rows, const float* ws_vals,
                              const int32_t* ws_ucount, const float* ws_absmax, const char* who, bool rest_ok = true);
// workgroups of `threads` for work_items, at least 1 and at most max_blocks (grid-stride kernels)
DQRM_HIDDEN int grid_for(int64_t work_items, int threads, int max_blocks = 2048);

// ---- The environment switches: one accessor each, all defined in one block of dqrm_host.hip,
// the only place of libdqrm that reads a DQRM_* variable ("Environment
// switches", lists them for users). Every switch is an A/B or test handle on a choice DESIGN.md 8
// measured; unset, each leaves the measured default. Unless said otherwise a switch is read once
// per process, on its first use.

// DQRM_WT_STORES=0|y|hand|all (default y): which once-written streams the kernels store
// write-through (16-B sc1 stores, dqrm_device.h st4_out): none / the forwards' y (WT_Y) / the
// N > 1 hand-over buffers (WT_HAND) / both. The launchers pass the bits on as a kernel argument
// or pick the kernel instance by them. dim: the tables' row length -- y rows under 128 B (D < 32)
// stay plain whatever the switch says: a 64-B row is half an L2 line, and written through it lost
// (Kaggle, D = 16: 27.36 vs 27.03 us per step; DESIGN.md 8, "write-through stores").
DQRM_HIDDEN uint32_t wt_stores(int dim);
// DQRM_APPLY=flat|slot|ranges|merge (default: DQRM_APPLY_AUTO): the apply kernel of
// dqrm_apply_sparse_update*, as a DQRM_APPLY_* kind. Seeds the process's choice on its first
// use; dqrm_set_apply_kernel overrides it. (tools/bench_apply_ranks.py)
DQRM_HIDDEN int env_apply();
// DQRM_FINALIZE=launch|inline (default 0 = per kernel: the flat apply kernels finalize the |W|
// hierarchy with a k_table_finalize launch, the slot kernels inside their launch): 1 / 2 force
// the launch / the in-launch hand-off for every kernel.
DQRM_HIDDEN int env_finalize();
// DQRM_FIN_FLAGGED=0 (default on): the finalize behind a flat apply visits only the tables the
// kernel flagged; 0 finalizes every table.
DQRM_HIDDEN bool env_fin_flagged();
// DQRM_FUSED_FWD=0 (default on): the next batch's forward rides in the update's launch
// (k_sgd_small, the one-launch local step, the merge apply); 0 keeps it a launch of its own.
DQRM_HIDDEN bool env_fused_fwd();
// DQRM_FIN_FWD=0 (default on): the flat apply's finalize and the next forward share one launch
// (k_finalize_fwd); 0 restores the two launches.
DQRM_HIDDEN bool env_fin_fwd();
// DQRM_LOCAL_FUSED=0 (default on): dqrm_emb_bwd_apply_local runs coalesce + update as one launch
// where it can; 0 always takes the two calls.
DQRM_HIDDEN bool env_local_fused();
// DQRM_QPACK=legacy (default off): dqrm_grad_quant_pack* runs the one-workgroup-per-slot
// k_quant_pack instead of dqrm_exchange.hip's kernel.
DQRM_HIDDEN bool env_qpack_legacy();
// DQRM_MERGE_KEYS=<n> (default 256; n <= 0 counts as unset): payload entries of all ranks per
// k_merge_pos workgroup, from which the merge apply sizes its chunks.
DQRM_HIDDEN int64_t env_merge_keys();
// DQRM_MERGE_DIAG=<n> (default 0): timing experiments only -- phases of k_merge_pos skipped, the
// results are then wrong.
DQRM_HIDDEN int env_merge_diag();
// DQRM_FLAT_DUAL=0|1|4 (default -1 = unset: by size, cap_total >= 512 * T): entries per lane
// group of the flat apply at 1 < N ranks: 0 one, 1 two (k_apply_flat2<.., 2>), 4 four. Read on
// EVERY call: tests switch it inside one process.
DQRM_HIDDEN int env_flat_dual();
// DQRM_GATE_SPIN=<polls> (default 2^20): polls of a table's gate before a fused forward's
// workgroup flags DQRM_ERRF_STALL (k_finalize_fwd, the merge apply's forward).
DQRM_HIDDEN uint32_t env_gate_spin();
// DQRM_STALL_SPIN=<polls> (default 2^20): rendezvous polls of the one-launch local step before a
// workgroup gives up and flags DQRM_ERRF_STALL (tests shorten it).
DQRM_HIDDEN uint32_t env_stall_spin();
// DQRM_SUBSLOTS=0 (default on): the one-launch local step halves the largest tables' slots
// between its spare workgroup groups; 0 leaves them idle.
DQRM_HIDDEN bool env_subslots();
// DQRM_SUBSLOT_ORDER=small (default: largest first): the smallest eligible tables get the
// sub-slots first.
DQRM_HIDDEN bool env_subslot_small_first();
// DQRM_TABLE_GROUPS=critical (default off): the one-launch local step deals the tables expected
// to end last onto the XCDs first.
DQRM_HIDDEN bool env_table_groups_critical();

// dqrm_linear.hip: what every dqrm_linear_* export rejects in a layer (quantized: the integer
// buffers and bit widths as well) and in an activation code. Texts are "<who>: <fault>".
DQRM_HIDDEN int check_linear(const dqrm_linear* l, int quantized, const char* who);
DQRM_HIDDEN int check_act(int act, const char* who);

// dqrm_mlp.hip: a stack as dqrm_mlp_fwd rejects it, and whether one of its layers quantizes per
// tensor (the fused SGD + requantize then takes a second launch and a workspace).
DQRM_HIDDEN int check_mlp(const dqrm_mlp* m, const char* who);
DQRM_HIDDEN bool has_tensor_layer(const dqrm_mlp* m);
// what dqrm_mlp_fwd_qact / _bwd_qact / _qact_prepare reject beyond check_mlp: a full-precision
// layer, per_channel anywhere but on the last layer, a null prev, out_scale array or entry
DQRM_HIDDEN int check_mlp_qact(const dqrm_mlp* m, const float* prev, float* const* out_scale, const char* who);

// dqrm_act.hip: the struct as dqrm_act_quant_fwd rejects it, and that call's launches for numel
// elements with a y (3, 2 or 1: see include/dqrm.h)
DQRM_HIDDEN int check_act_quant(const dqrm_act_quant* q, const char* who);
DQRM_HIDDEN int act_quant_fwd_launches(const dqrm_act_quant* q, int64_t numel);

// dqrm_kernels.hip, for the whole-model step (dqrm_model.hip), which validates its embedding
// stage before its first launch: everything dqrm_emb_fwd and dqrm_emb_bwd_sgd / _sgd_fwd reject,
// apart from the out / dy pointers and strides, which that caller lays out itself. batch == NULL:
// the set alone. training == 0: the forward's checks only. next: the batch whose forward follows
// the update (nullable).
DQRM_HIDDEN int emb_check(const dqrm_table_set* set, const dqrm_batch* batch, const dqrm_batch* next, int bits,
                          uint32_t fwd_flags, int repack_bits, int training, const char* who);
// launches of dqrm_emb_bwd_sgd (next == NULL) / dqrm_emb_bwd_sgd_fwd on arguments that passed
// emb_check
DQRM_HIDDEN int emb_bwd_sgd_launches(const dqrm_table_set* set, const dqrm_batch* batch, const dqrm_batch* next,
                                     uint32_t fwd_flags);

// dqrm_rowwise.hip, for dqrm_model_fwd_rowwise (dqrm_model.hip), which validates its embedding
// stage before its first launch: everything dqrm_rowwise_set_fwd rejects in the set and (batch
// nullable: the set alone) in the batch, apart from the out pointer and strides, which that caller
// lays out itself.
DQRM_HIDDEN int rowwise_set_check(const dqrm_rowwise_set* set, const dqrm_batch* batch, const char* who);

// The coalesce backward of a Criteo-form batch (DQRM_BATCH_POOLING_ONE: table t's lookups
// are idx[t*B, (t+1)*B), bag b = lookup b), written into the caller's coalesced-gradient
// workspace (include/dqrm.h, dqrm_emb_bwd_coalesce).
struct CoalesceArgs {
    const int64_t* meta;        // [4][T] row_base, num_rows, blk_base, sblk_base
    int T;
    int D;
    int64_t B;                  // lookups (= bags) per table
    const int64_t* idx;         // [T][B]
    const float* dy;            // dy[t*dst_t + b*dst_b + d]
    int64_t dst_t, dst_b;
    const float* scale;         // [T] forward scale (STE)
    int ste;
    uint32_t* err;
    const int64_t* ws_cap_base; // [T*S+1]
    int32_t* ws_rows;
    float* ws_vals;
    int32_t* ws_ucount;
    float* ws_absmax;
};

// The single-rank update fused behind the coalesce (dqrm_emb_bwd_apply_local): quantize the
// coalesced rows with the table's scale, SGD into W and keep the |W| hierarchy exact
// (dqrm_apply_local's arithmetic), inside the same launch.
struct LocalApplyArgs {
    float* W;
    uint8_t* packed;
    float* rowmax;
    float* blkmax;
    float* sblkmax;
    uint8_t* sdirty;
    uint8_t* bdirty;
    float* tmax;
    const float* pscale;
    uint32_t* sync;             // [T * DQRM_SYNC_STRIDE]: arrival counters of the table's workgroups
    float* s_avg;               // [T] the table scale the update used
    int bits;
    float nlr;                  // -lr
    int repack;
    // sub-slots (host-planned, dqrm_coalesce.hip): spare group e serves table sub_table[e]
    // (-1: idle); bit t of sub_mask = table t's slots are halved between two workgroups
    uint32_t sub_mask;
    int8_t sub_table[32];
    // group g < T serves table table_of_group[g] when group_perm (host-planned, A/B
    // DQRM_TABLE_GROUPS=critical: the tables expected to end last on the XCDs dealt first)
    int8_t table_of_group[32];
    int group_perm;
    // rendezvous polls before a workgroup gives up (DQRM_ERRF_STALL; its rows are then applied
    // by the table's last-arriving workgroup); the host sets it (DQRM_STALL_SPIN, default 2^20)
    uint32_t spin_limit;
    // the next batch's forward behind the update (dqrm_emb_bwd_apply_fwd_local; fwd_idx null:
    // none): Criteo-form indices [T][B] (the same B), out[t*fwd_ost_t + b*fwd_ost_b + d],
    // dqrm_emb_fwd's bits and flags (DQRM_FWD_REFRESH_SCALE / DQRM_FWD_FULL_PRECISION)
    const int64_t* fwd_idx;
    float* fwd_out;
    int64_t fwd_ost_t, fwd_ost_b;
    float* fwd_scale;           // [T] the forward scale: written (refresh) or read (held)
    int fwd_bits;
    uint32_t fwd_flags;
};
constexpr int kSubTables = 32;  // LocalApplyArgs::sub_table entries

// largest B the Criteo-form coalesce kernel takes (larger batches use the general kernel)
constexpr int64_t kCoalesceMaxB = 4096;
// largest table count the fused coalesce + update runs with: its (T+7)/8*64 workgroups of
// 1024 threads (one per CU: 156 KiB LDS) must all be resident at once, since a table's
// workgroups wait for each other's gradient maxima
constexpr int kCoalesceApplyMaxT = 32;

// Whether the fused form's grid of T tables can be resident at once on the current device
// from `stream`: workgroups per CU (occupancy query) x CUs >= the grid, and the stream's CU
// mask enables every CU. Device properties are queried once per device.
bool coalesce_apply_resident(int T, hipStream_t stream);

// Sub-slot plan of the fused form (la->sub_mask / sub_table) from the host row counts
// (nullable: no sub-slots). DQRM_SUBSLOTS=0 in the environment disables them (A/B).
void plan_sub_slots(const int64_t* num_rows_host, int T, LocalApplyArgs* la);

// launches k_coalesce_p1 (dqrm_coalesce.hip); la != nullptr: the fused update as well
// (hipErrorInvalidValue if !coalesce_apply_resident). Returns the HIP error of the launch.
hipError_t launch_coalesce_pool1(const CoalesceArgs& a, const LocalApplyArgs* la, hipStream_t stream);

// K6 with row ranges owned per workgroup (dqrm_apply.hip, DQRM_APPLY_RANGES): the gathered
// payloads decoded, summed over ranks, applied, and the |W| hierarchy finalized in-launch.
struct RangeApplyArgs {
    float* W;
    uint8_t* packed;
    float* rowmax;
    float* blkmax;
    float* sblkmax;
    uint8_t* sdirty;
    uint8_t* bdirty;
    float* tmax;
    uint32_t* sync;
    const float* pscale;
    const int64_t* meta;
    uint32_t* err;
    const int64_t* cap_base;
    int64_t cap_total;
    const unsigned char* payloads;  // rank r's payload at payloads + r * rank_pitch
    int64_t rank_pitch;
    int N;
    int T;
    int D;
    int bits;
    const float* s_avg;
    float nlr;
    int mode;
    int repack;
    int K;                          // chunks per row-range slot
};
hipError_t launch_apply_ranges(const RangeApplyArgs& a, hipStream_t stream);

// K6 with the ranks' rows merged on chip (dqrm_apply_merge.hip, DQRM_APPLY_MERGE): k_merge_pos
// (workgroups own block-aligned row ranges, K_t chunks per row-range slot of table t, locate every
// entry's row in the other ranks' runs in LDS) writes the positions; k_apply_pos updates, finalizes
// the |W| hierarchy in-launch and (fwd_idx) runs the next batch's forward behind per-table gates.
constexpr int kMergeMaxRanks = 16;
constexpr int kMergeMaxTables = 64;
struct MergeApplyArgs {
    float* W;
    uint8_t* packed;
    float* rowmax;
    float* blkmax;
    float* sblkmax;
    uint8_t* sdirty;
    uint8_t* bdirty;
    float* tmax;
    uint32_t* sync;
    const float* pscale;
    const int64_t* meta;
    uint32_t* err;
    const int64_t* cap_base;
    int64_t cap_total;
    const unsigned char* payloads;  // rank r's payload at payloads + r * rank_pitch
    int64_t rank_pitch;
    int N;
    int T;
    int D;
    int bits;
    const float* s_avg;
    float nlr;
    int mode;
    int repack;
    int32_t* pos;                     // N > 1: [N][cap_total][N] workspace (apply_workspace_bytes)
    int gx;                           // k_apply_pos: entry chunks per (table, rank)
    int kt[kMergeMaxTables];          // k_merge_pos: chunks per row-range slot of table t
    int kbase[kMergeMaxTables + 1];   //   first workgroup of table t (SPLIT * kt prefix)
    // the next batch's forward in the same launch (fwd_idx null: none): Criteo-form indices
    // [T][fwd_B], out[t*fwd_ost_t + b*fwd_ost_b + d], dqrm_emb_fwd's bits / flags
    // (DQRM_FWD_REFRESH_SCALE, DQRM_FWD_FULL_PRECISION); fwd_gx workgroups per table
    const int64_t* fwd_idx;
    int64_t fwd_B;
    float* fwd_out;
    int64_t fwd_ost_t, fwd_ost_b;
    float* fwd_scale;
    int fwd_bits;
    uint32_t fwd_flags;
    int fwd_gx;
    uint32_t spin_limit;              // gate polls before a forward workgroup flags DQRM_ERRF_STALL
    uint32_t wt;                      // wt_stores() bits (WT_Y: y write-through)
    int diag;                         // DQRM_MERGE_DIAG (timing experiments only; 0 in normal use)
};
hipError_t launch_apply_merge(const MergeApplyArgs& a, hipStream_t stream);
int merge_forward_gx(int64_t B);
size_t apply_workspace_bytes(int num_ranks, int64_t cap_total);

}  // namespace dqrm_internal
