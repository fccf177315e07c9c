/*
 * dqrm.h — C ABI of libdqrm, the MI355X-native (gfx950 / CDNA4) implementation of
 * DQRM's data-parallel QAT step for embedding tables.
 *
 * Reference: YangZhou08/Deep_Quantized_Recommendation_Model_DQRM @ 2024-10-24.
 * Each entry point below names the reference interface it replaces (file:line).
 *
 * Conventions
 *  - Plain C: pointers, sizes, enums. No torch types. Every device pointer is a HIP
 *    device allocation owned by the caller; the library never allocates or frees
 *    caller memory and keeps no global device state.
 *  - Every call is stream-ordered on the hipStream_t passed as `void* stream`
 *    (NULL = the legacy default stream). No call synchronises the host except
 *    dqrm_read_errors().
 *  - Every call returns an int status: 0 = ok, <0 = error (see DQRM_E_*). The message
 *    of the last failing call on the calling thread is returned by dqrm_last_error().
 *    No C++ exception crosses the ABI.
 *  - Shapes: T tables, D = embedding dim (same for all tables, D % 4 == 0, D <= 256),
 *    B = bags per table per call, L_t = lookups of table t.
 *
 * Resident table state (one "table set" = all T tables of a model, one slab each):
 *    W        f32 [R][D]            FP32 master rows, table t = rows [row_base[t], +num_rows[t])
 *    packed   u8  [R][D/2]          INT4 rows, offset-binary nibbles (q+8), element 2j in the
 *                                   low nibble of byte j (FBGEMM/torch 4-bit rowwise order);
 *                                   nullable when the packed path is unused
 *    rowmax   f32 [R]               max_d |W[r][d]|
 *    blkmax   f32 [NB]              max of rowmax over 256-row blocks   (blk_base[t] per table)
 *    sblkmax  f32 [NS]              max of blkmax over 256-block (65536-row) superblocks
 *    tmax     f32 [T]               max of sblkmax over the table = max |W_t|
 *    scale    f32 [T]               embedding scale s_t used by the latest forward
 *    pscale   f32 [T]               scale the packed rows were built with (NaN = never)
 *    meta     i64 [4][T]            row_base, num_rows, blk_base, sblk_base (device copy)
 *
 *  The max hierarchy makes the reference's per-step full-table min/max
 *  (quant_utils.py:177-178, called every training forward at
 *  quant_modules_not_quantize_grad.py:337) exact and O(touched rows).
 */
#ifndef DQRM_H_
#define DQRM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQRM_ABI_VERSION 12 /* 2: dqrm_table_set.bdirty, dqrm_set_apply_kernel, dqrm_apply_local;
                               3: backward workspace (dqrm_bwd_workspace_bytes), no per-slot key cap;
                               4: dqrm_table_set.sync (in-launch hierarchy finalize), padded flags;
                               5: dqrm_emb_bwd_apply_local (coalesce + local update, one launch);
                               6: residency-checked one launch (dqrm_bwd_apply_local_is_one_launch),
                                  dqrm_checksum64 mixes the full 64-bit position,
                                  dqrm_table_set.num_rows_host;
                               7: dqrm_emb_fwd_after_update;
                               8: dqrm_comm (RCCL communicator owned by libdqrm), dqrm_exchange
                                  (the N > 1 exchange as two calls), dqrm_emb_bwd_lookup_grad_presum;
                               9: dqrm_emb_bwd_apply_fwd_local (the next batch's forward behind the
                                  one-launch update), dqrm_bwd_apply_fwd_local_is_one_launch,
                                  dqrm_emb_bwd_sgd_fwd;
                              10: dqrm_comm_init_external (a caller-served all-gather under the
                                  same exchange orchestration), dqrm_comm_size,
                                  dqrm_bwd_sgd_fwd_is_one_launch, DQRM_APPLY_MERGE,
                                  dqrm_apply_sparse_update_fwd, dqrm_apply_fwd_is_one_launch,
                                  dqrm_apply_workspace_bytes, dqrm_exchange.apply_ws,
                                  dqrm_exchange_apply_fwd;
                              11: the flat apply's finalize and the next forward in one launch
                                  (dqrm_apply_sparse_update_fwd), dqrm_apply_fwd_form;
                              12: dqrm_linear (QuantLinear on the f32-input MFMA): dqrm_linear_wquant,
                                  dqrm_linear_fwd, dqrm_linear_bwd;
                                  added within 12 (new symbols only, no existing signature or
                                  struct changed): dqrm_interact (the dot feature interaction):
                                  dqrm_interact_out_features, dqrm_interact_scale,
                                  dqrm_interact_fwd, dqrm_interact_bwd;
                                  likewise within 12: the MLP's activation fused into the layer,
                                  DQRM_ACT_*, dqrm_linear_fwd_act, dqrm_linear_bwd_act;
                                  likewise within 12: activation quantization, dqrm_act_quant
                                  (QuantAct): dqrm_act_quant_workspace_bytes, dqrm_act_quant_fwd,
                                  dqrm_act_quant_bwd; and the layer's integer-activation branch:
                                  dqrm_linear_wquant_qact, dqrm_linear_fwd_qact,
                                  dqrm_linear_bwd_qact;
                                  likewise within 12: the loss head, dqrm_loss (DLRMLoss),
                                  DQRM_LOSS_*: dqrm_loss_fwd, dqrm_loss_bwd;
                                  likewise within 12: a whole MLP stack per call, dqrm_mlp
                                  (MLPStack): dqrm_mlp_fwd, dqrm_mlp_bwd_scratch_bytes,
                                  dqrm_mlp_bwd, dqrm_mlp_sgd_workspace_bytes, dqrm_mlp_sgd;
                                  likewise within 12: the whole model per call, dqrm_model (DQRMNet):
                                  dqrm_mlp_sgd_multi_workspace_bytes, dqrm_mlp_sgd_multi,
                                  dqrm_model_workspace_bytes, dqrm_model_workspace_layout,
                                  dqrm_model_fwd, dqrm_model_step, dqrm_model_step_launches;
                                  likewise within 12: the test loop's metrics, dqrm_metrics
                                  (DLRMMetrics): dqrm_metrics_reset, dqrm_metrics_update,
                                  dqrm_metrics_workspace_bytes, dqrm_metrics_finish,
                                  dqrm_metrics_finish_launches;
                                  likewise within 12: the quantized model served from row-wise
                                  tables, dqrm_rowwise_set (DQRMNet.quantize_embedding):
                                  dqrm_rowwise_set_fwd, dqrm_model_fwd_rowwise,
                                  dqrm_model_fwd_rowwise_workspace_bytes,
                                  dqrm_model_fwd_rowwise_workspace_layout,
                                  dqrm_model_fwd_rowwise_launches;
                                  likewise within 12: the MLP half of the simulated-DP buffer
                                  (sgd_quantized_gradients): dqrm_dense_ec_accumulate,
                                  dqrm_dense_sim_update;
                                  likewise within 12: quantize_activation models on the stack and
                                  the whole-model calls, dqrm_model_qact: dqrm_mlp_qact_prepare,
                                  dqrm_mlp_fwd_qact, dqrm_mlp_bwd_qact, dqrm_model_fwd_qact,
                                  dqrm_model_step_qact, dqrm_model_qact_workspace_bytes,
                                  dqrm_model_qact_workspace_layout,
                                  dqrm_model_qact_step_launches;
                                  likewise within 12: the LSQ and PACT embedding quantizers
                                  (QuantEmbeddingBagLSQ / QuantEmbeddingBagPACT): dqrm_emb_fwd_lsq,
                                  dqrm_emb_bwd_lsq, dqrm_emb_bwd_lsq_workspace_bytes,
                                  dqrm_emb_fwd_pact, dqrm_emb_fwd_lsq_launches,
                                  dqrm_emb_bwd_lsq_launches, dqrm_emb_fwd_pact_launches */

/* status codes */
#define DQRM_OK            0
#define DQRM_E_INVALID    -1   /* bad argument (shape, null pointer, unsupported bits) */
#define DQRM_E_HIP        -2   /* HIP runtime error */
#define DQRM_E_CAPACITY   -3   /* a size exceeds this build's index range (e.g. max_lookups >= 2^30) */
#define DQRM_E_WORKSPACE  -4   /* workspace too small */

/* device-side error flags accumulated in dqrm_table_set.err (read with dqrm_read_errors) */
#define DQRM_ERRF_INDEX    1u  /* an index was outside [0, num_rows[t]) (reference: IndexError) */
#define DQRM_ERRF_OFFSET   2u  /* offsets not non-decreasing / outside [0, L_t] */
#define DQRM_ERRF_OVERFLOW 4u  /* a table had more lookups than dqrm_batch.max_lookups promised, or a
                                      caller-sized workspace / payload was too small */
#define DQRM_ERRF_STALL    8u  /* the workgroups of a fused launch could not all be resident at once
                                  (dqrm_emb_bwd_apply_local): its update is incomplete */

#define DQRM_BLOCK_ROWS   256     /* rows per blkmax entry */
#define DQRM_SBLOCK_ROWS  65536   /* rows per sblkmax entry */
#define DQRM_TABLE_SPLIT  8       /* workgroups (row-range slots) per table in the backward */
#define DQRM_SYNC_STRIDE  64      /* uint32 words between two tables' arrival counters */
#define DQRM_SLOT_KEYS    8192    /* merged payload entries the slot apply kernel sorts on chip
                                     (a fuller slot is applied by the flat method instead) */

/* Resident state of T tables. All pointers are device pointers. */
typedef struct dqrm_table_set {
    int32_t  num_tables;      /* T */
    int32_t  dim;             /* D */
    int64_t  total_rows;      /* R = sum num_rows */
    int64_t  total_blocks;    /* NB */
    int64_t  total_sblocks;   /* NS */
    float*   W;
    uint8_t* packed;          /* nullable */
    float*   rowmax;
    float*   blkmax;
    float*   sblkmax;
    float*   tmax;
    float*   scale;
    float*   pscale;
    const int64_t* meta;      /* [4][T]: row_base, num_rows, blk_base, sblk_base */
    uint32_t* err;            /* 1 word, device-side error flags */
    uint32_t* tflags;         /* [T] scratch (repack decision), library-internal */
    uint8_t*  sdirty;         /* [NS] zero-initialised scratch (superblock rescan flags); the
                                 allocation is readable up to the next 4-byte boundary */
    uint8_t*  bdirty;         /* [NB] zero-initialised scratch (block rescan flags), same padding */
    uint32_t* sync;           /* [T * DQRM_SYNC_STRIDE] zero-initialised scratch: per-table
                                 arrival counters of the updating kernels (the last workgroup
                                 of a table finalizes its |W| hierarchy inside the launch), one
                                 per 256 bytes; library-internal */
    const int64_t* num_rows_host; /* nullable HOST array [T]: the tables' row counts (meta's
                                 second row), for host-side launch planning (the one-launch local
                                 step gives its spare workgroups to the largest tables) */
} dqrm_table_set;

/* A batch of lookups for all T tables, in the reference's per-table
 * (lS_i[t], lS_o[t]) form (dlrm_data_pytorch.py:328-345, 1099-1157), concatenated:
 *   idx      i64 [sum_t L_t]  table t's indices at [idx_base[t], idx_base[t+1])
 *   off      i64 [T][B]       bag b of table t = idx_base[t] + [off[t][b], off[t][b+1])
 *                             (last bag ends at L_t), exactly nn.EmbeddingBag offsets
 *   idx_base i64 [T+1]        device copy
 * max_lookups must bound every L_t: it sizes the backward workspace (a table with more
 * lookups is skipped and flags DQRM_ERRF_OVERFLOW). There is no other per-batch limit. */
typedef struct dqrm_batch {
    const int64_t* idx;
    const int64_t* off;
    const int64_t* idx_base;
    int64_t  num_bags;        /* B */
    int64_t  max_lookups;     /* host upper bound on any L_t (capacity planning) */
    uint32_t flags;           /* DQRM_BATCH_* */
    uint32_t reserved;
} dqrm_batch;

/* Criteo form (dlrm_data_pytorch.py:328-345): every table has L_t == B (so idx_base[t] ==
 * t * B) and off[t][b] == b, i.e. bag b is lookup b. The kernels then read neither the
 * offsets nor idx_base. */
#define DQRM_BATCH_POOLING_ONE 1u

/* forward flags */
#define DQRM_FWD_REFRESH_SCALE 1u  /* s_t = clamp(tmax_t, 1e-8)/(2^(bits-1)-1), write scale[] */
#define DQRM_FWD_USE_PACKED    2u  /* single-lookup bags read INT4 rows (valid iff pscale==scale) */
#define DQRM_FWD_FULL_PRECISION 4u /* full_precision_flag: plain FP32 sum, no fake-quant */
#define DQRM_FWD_NT_STORE      16u /* stream the output with non-temporal stores (packed path) */

/* ---------------------------------------------------------------------------------
 * Table maintenance
 * ------------------------------------------------------------------------------ */

/* Full recompute of rowmax/blkmax/sblkmax/tmax from W (first forward, after
 * load_state_dict, after weight_syncc). Replaces the full-table scan of
 * quant_utils.py:141-194 (symmetric_linear_quantization_param_two). */
int dqrm_refresh_absmax(const dqrm_table_set* set, void* stream);

/* Periodic scale refresh + conditional repack (the stringified periodic-update path
 * quant_modules_not_quantize_grad.py:303-315,331-363). For each table:
 *   s_t = clamp(tmax_t, 1e-8) / (2^(bits-1)-1)   -> scale[t]
 *   if packed != NULL and pscale[t] != s_t: repack every row of t with s_t, pscale[t] = s_t.
 * Device-side decision; no host sync. bits must be 4 for repacking. */
int dqrm_refresh_scale_and_pack(const dqrm_table_set* set, int bits, void* stream);

/* ---------------------------------------------------------------------------------
 * Forward: fused multi-table INT4 fake-quant EmbeddingBag
 * Replaces QuantEmbeddingBagTwo.forward (quant_modules_not_quantize_grad.py:317-398)
 * called once per table by DLRM_Net.apply_emb (dlrm_s_pytorch_single_gpu.py:609-674):
 *   out = embedding_bag(idx, off, mode="sum")              (:367)
 *   q   = clamp(round(1/s * out + 0), -2^(b-1), 2^(b-1)-1)  (quant_utils.py:101,343)
 *   y   = q * s                                             (:393)
 * out[t][b][d] is written at out + t*out_stride_t + b*out_stride_b + d (floats).
 * Bags with one lookup may be served from the INT4 packed rows (bit-identical values
 * when pscale == scale); every other bag is summed in FP32 in bag order.
 * ------------------------------------------------------------------------------ */
int dqrm_emb_fwd(const dqrm_table_set* set, const dqrm_batch* batch, int bits,
                 uint32_t flags, float* out, int64_t out_stride_t, int64_t out_stride_b,
                 void* stream);

/* ---------------------------------------------------------------------------------
 * Backward workspace. The three backward calls below (SGD, coalesce, local update) sort
 * the lookups of every (table, row-range slot) by row on the device (in LDS up to 4096
 * lookups, in this workspace beyond) and process the distinct rows from a device-built
 * work list. Its size depends only on the table count and dqrm_batch.max_lookups: 16 bytes
 * up to 4096 lookups per table, T * DQRM_TABLE_SPLIT * max_lookups * 20 bytes beyond (each
 * of a table's row-range slots gets a spill region for all of the table's lookups, since a
 * slot's share is only known on the device; e.g. 26 tables x 1 M lookups = 4.2 GB).
 * Returns the bytes needed (0 on bad arguments). The workspace must be 16-B aligned; it
 * needs no initialisation (one call at a time per workspace).
 * ------------------------------------------------------------------------------ */
size_t dqrm_bwd_workspace_bytes(int num_tables, int64_t max_lookups);

/* ---------------------------------------------------------------------------------
 * Single-GPU backward + SGD, fused (no sparse gradient materialised).
 * Replaces: SymmetricQuantFunction.backward (quant_utils.py:349-363) + autograd of q*s,
 * EmbeddingBag sparse backward, and torch.optim.SGD.step on the sparse grad
 * (dlrm_s_pytorch_single_gpu.py:1736-1750,1943-1950). Per lookup i of row r, in lookup
 * order:  g' = (dy[bag(i)] * s) / s ;  W[r] = fma(g', -lr, W[r])   (torch CPU order).
 * ste = 0 skips the (g*s)/s step (forward ran with full_precision_flag).
 * Then rowmax/blkmax/sblkmax/tmax of touched rows, and (if packed != NULL and
 * repack_bits == 4) the touched INT4 rows with pscale.
 * ------------------------------------------------------------------------------ */
int dqrm_emb_bwd_sgd(const dqrm_table_set* set, const dqrm_batch* batch,
                     const float* dy, int64_t dy_stride_t, int64_t dy_stride_b,
                     int ste, float lr, int repack_bits, void* workspace, size_t workspace_bytes,
                     void* stream);

/* dqrm_emb_bwd_sgd on `batch`, then dqrm_emb_fwd(set, next, fwd_bits, fwd_flags, out, ...) on
 * the NEXT batch, with the same results as the two calls: the single-GPU driver's SGD step
 * (dlrm_s_pytorch_single_gpu.py:1943-1950) and the next apply_emb (:609-674), adjacent in its
 * loop. When the update takes the small-batch kernel (one workgroup per table, B <= 512
 * lookups) and `next` is a Criteo-form batch of the same size without DQRM_FWD_USE_PACKED,
 * each table's workgroup runs the next forward of that table itself right after its update:
 * one launch per step. Otherwise the two calls run. (A table whose batch overflows the
 * declared max_lookups is skipped and flagged, DQRM_ERRF_OVERFLOW, by the update and, in the
 * one-launch form, by its forward too.) */
int dqrm_emb_bwd_sgd_fwd(const dqrm_table_set* set, const dqrm_batch* batch, const float* dy,
                         int64_t dy_stride_t, int64_t dy_stride_b, int ste, float lr, int repack_bits,
                         void* workspace, size_t workspace_bytes, const dqrm_batch* next, int fwd_bits,
                         uint32_t fwd_flags, float* out, int64_t out_stride_t, int64_t out_stride_b,
                         void* stream);

/* 1 if dqrm_emb_bwd_sgd_fwd would run the SGD of `batch` and the forward of `next` as ONE
 * launch (the small-batch kernel takes the update and `next` is a Criteo-form batch of the
 * same size without DQRM_FWD_USE_PACKED), 0 if as two launches, <0 on bad arguments. */
int dqrm_bwd_sgd_fwd_is_one_launch(const dqrm_table_set* set, const dqrm_batch* batch, const dqrm_batch* next,
                                   uint32_t fwd_flags);

/* ---------------------------------------------------------------------------------
 * Data-parallel gradient path (sgd_quantized_gradients_parallel_comm.py)
 *
 * Coalesced-gradient workspace (per rank). Slot k = t * DQRM_TABLE_SPLIT + s holds the
 * coalesced rows of table t that fall in row range s (ascending, unique):
 *   ws_cap_base i64 [T*S+1] (device)  slot k owns entries [ws_cap_base[k], ws_cap_base[k+1])
 *   ws_rows     i32 [WCAP]            local row ids
 *   ws_vals     f32 [WCAP][D]         coalesced sums
 *   ws_ucount   i32 [T*S]             entries used per slot
 *   ws_absmax   f32 [T*S]             partial maxima of |vals|: the max over table t's S
 *                                     entries is max |vals_t| (the local scale's input)
 * dqrm_coalesce_slot_caps() gives the slot capacities (host).
 * ------------------------------------------------------------------------------ */

/* Host helper: slot capacities cap[t*S+s] = min(max_lookups, rows in slot s of table t)
 * (a slot can never hold more distinct rows than that);
 * writes the exclusive prefix into ws_cap_base_host[T*S+1]; returns WCAP (>= 0). */
int64_t dqrm_coalesce_slot_caps(const int64_t* num_rows_host, int num_tables, int64_t max_lookups,
                                int64_t* ws_cap_base_host);

/* STE backward + EmbeddingBag sparse backward + grad.coalesce() (s_q_g_p_c.py:859),
 * plus the per-slot max |value| feeding the local scale
 * s_loc[t] = clamp(max|vals_t|, 1e-8) / (2^(bits-1)-1) (:861, quant_utils.py:141-194). */
int dqrm_emb_bwd_coalesce(const dqrm_table_set* set, const dqrm_batch* batch,
                          const float* dy, int64_t dy_stride_t, int64_t dy_stride_b,
                          int ste, const int64_t* ws_cap_base, int32_t* ws_rows, float* ws_vals,
                          int32_t* ws_ucount, float* ws_absmax, void* workspace, size_t workspace_bytes,
                          void* stream);

/* dqrm_emb_bwd_coalesce with every lookup's gradient divided by `divisor` before the
 * coalescing sum: values = sum over the row's lookups, in lookup order, of
 * ((dy*s)/s) / divisor -- the unquantized simulated-DP buffer of sgd_quantized_gradients.py:88-91
 * (embedding_grad_buffer.add_(grad / number_of_gpus); .coalesce()) when the batch holds the
 * N micro-steps' lookups back to back. Always the general (sorting) kernel; divisor 1 is
 * dqrm_emb_bwd_coalesce. */
int dqrm_emb_bwd_coalesce_scaled(const dqrm_table_set* set, const dqrm_batch* batch,
                                 const float* dy, int64_t dy_stride_t, int64_t dy_stride_b,
                                 int ste, int divisor, const int64_t* ws_cap_base, int32_t* ws_rows,
                                 float* ws_vals, int32_t* ws_ucount, float* ws_absmax, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* Per-lookup (uncoalesced) sparse gradient, the COO nn.EmbeddingBag(mode="sum",
 * sparse=True) produces (embedding_bag_backward, sparse branch): for every lookup j of
 * table t, in lookup order, rows[j] = row_base[t] + idx[j] (slab row) and
 * vals[j][:] = (dy[t, bag(j)] * s_t) / s_t (ste != 0, quant_utils.py:349-363; s_t =
 * set->scale[t], the forward's scale) or dy[t, bag(j)]. j runs over the batch's flat
 * lookup positions (idx_base). The grad_mode="sparse" module hands this to
 * torch.optim.SGD (dlrm_s_pytorch_single_gpu.py:1943-1950), which then adds lookup by
 * lookup as with the reference's own embedding grad. rows i64 [L], vals f32 [L][D]. */
int dqrm_emb_bwd_lookup_grad(const dqrm_table_set* set, const dqrm_batch* batch, const float* dy,
                             int64_t dy_stride_t, int64_t dy_stride_b, int ste, int64_t* rows, float* vals,
                             void* stream);

/* Rows of W rewritten outside libdqrm -- torch.optim.SGD stepping on the
 * dqrm_emb_bwd_lookup_grad COO: recompute their row maxima, re-reduce their blocks,
 * superblocks and table maxima (the next refreshing forward's scale is then the full-table
 * max again, quant_utils.py:141-194) and, repack_bits == 4, repack their INT4 rows with the
 * frozen packing scale. rows: slab rows (device i64 [n], duplicates allowed). */
int dqrm_rows_changed(const dqrm_table_set* set, const int64_t* rows, int64_t n, int repack_bits, void* stream);

/* dqrm_rows_changed(set, rows, n, repack_bits) followed by dqrm_emb_fwd(set, batch, ...),
 * same results: the per-table module's sync after a torch.optim.SGD step on its COO grad
 * and its next forward (q_m_n_q_g.py:317-398 with the full-table scale of
 * quant_utils.py:141-194). A one-table set with a small batch (bags * D/4 <= 4096, n <= 4096,
 * FP32 rows, no repack) runs both as ONE single-workgroup launch; anything else as the two
 * calls. n == 0 is dqrm_emb_fwd. */
int dqrm_emb_fwd_after_update(const dqrm_table_set* set, const dqrm_batch* batch, int bits, uint32_t flags,
                              float* out, int64_t out_stride_t, int64_t out_stride_b, const int64_t* rows,
                              int64_t n, int repack_bits, void* stream);

/* Wire payload of one rank (bytes), produced by dqrm_grad_quant_pack:
 *   [counts i32 T*S | pad to 16] [rows i32 CAP | pad to 16] [vals CAP*D elems of
 *   int8 (bits<=8) / int16 (bits<=16) / f32 (bits==32, unquantized path)]
 * counts[t*S+s] = entries of table t in row-range slot s (S = DQRM_TABLE_SPLIT); table t's
 * entries sit at [cap_base[t], cap_base[t] + sum_s counts[t*S+s]), rows ascending, slot
 * after slot (so a receiving slot finds its entries without searching). */
size_t dqrm_payload_bytes(int num_tables, int64_t cap_total, int dim, int grad_bits);

/* Scale average + quantize-pack (s_q_g_p_c.py:861-869). absmax_all = the N ranks'
 * ws_absmax gathered [N][T*S]. Per table:
 *   s_r  = clamp(max_s absmax_all[r][t*S+s], 1e-8) / (2^(bits-1)-1)     (rank r's scale)
 *   s    = (((s_{N-1} + s_{N-2}) + ...) + s_0) * (1/N)
 *          (Gloo's one-element allreduce order; identical on every rank; -> s_avg)
 *   q    = clamp(round(1/s * v + 0), -2^(bits-1), 2^(bits-1)-1)  (quant_utils.py:101,343)
 * and the slots are compacted into the dense payload. grad_bits = 32 copies FP32 values
 * (emb_grad_quantized=False path, :319-327); absmax_all / s_avg may then be NULL. */
int dqrm_grad_quant_pack(int num_tables, int dim, const int64_t* ws_cap_base, int64_t ws_cap_total,
                         const int32_t* ws_rows, const float* ws_vals, const int32_t* ws_ucount,
                         const float* absmax_all, int num_ranks, int grad_bits,
                         const int64_t* cap_base, int64_t cap_total, float* s_avg, void* payload,
                         void* stream);

/* dqrm_grad_quant_pack with the ranks' max|grad| rows absmax_pitch floats apart
 * (absmax_all[r * absmax_pitch + t*S + s]; >= T*S): one all-gather of several table sets'
 * concatenated ws_absmax serves every set (the DP hooks over a ModuleList of per-table
 * modules, sgd_quantized_gradients_parallel_comm.py). payload 16-B aligned. */
int dqrm_grad_quant_pack_strided(int num_tables, int dim, const int64_t* ws_cap_base, int64_t ws_cap_total,
                                 const int32_t* ws_rows, const float* ws_vals, const int32_t* ws_ucount,
                                 const float* absmax_all, int64_t absmax_pitch, int num_ranks, int grad_bits,
                                 const int64_t* cap_base, int64_t cap_total, float* s_avg, void* payload,
                                 void* stream);

/* Ranking-range mixed-precision gradients (grad_precision_and_scale
 * s_q_g_p_c.py:158-255 decides a bit width per table: 0, 8 or 32). Quantize-pack with a
 * per-table bit width and scale (quantize_emb_grad_two, :836-848):
 *   table_bits[t] in 2..8 : q = clamp(round(1/table_scale[t] * v + 0), -2^(b-1), 2^(b-1)-1)
 *   table_bits[t] 0 or 32: the table sends no entries (grad_update_parallel_comm skips it, :280-289)
 * The payload layout is that of grad_bits = 8 (int8 values); apply it with
 * dqrm_apply_sparse_update(mode DQRM_UPD_DP, grad_bits 8, s_avg = table_scale). */
int dqrm_grad_quant_pack_ranked(int num_tables, int dim, const int64_t* ws_cap_base, int64_t ws_cap_total,
                                const int32_t* ws_rows, const float* ws_vals, const int32_t* ws_ucount,
                                const int32_t* table_bits, const float* table_scale, const int64_t* cap_base,
                                int64_t cap_total, void* payload, void* stream);

/* Local (uncommunicated) update of the ranking-range 32-bit tables,
 * weight_update_parallel_comm :615-616  W.add_(-lr * grad)  with grad the rank's own sparse
 * gradient: per lookup, in lookup order, W[r] = W[r] + (g' * -lr) with g' = (dy*s)/s
 * (ste != 0), the product rounded separately. Only tables with table_mask[t] != 0
 * (NULL = all) are touched; rowmax/blkmax/sblkmax/tmax and (repack_bits == 4) packed rows
 * are maintained as in dqrm_emb_bwd_sgd. */
int dqrm_emb_local_update(const dqrm_table_set* set, const dqrm_batch* batch, const float* dy,
                          int64_t dy_stride_t, int64_t dy_stride_b, int ste, float lr, const int32_t* table_mask,
                          int repack_bits, void* workspace, size_t workspace_bytes, void* stream);

/* update modes for dqrm_apply_sparse_update */
#define DQRM_UPD_DP        0  /* v = ((Q * (1/N)) * s) ; W += -lr * v   (s_q_g_p_c.py:885,618-622) */
#define DQRM_UPD_SIMULATED 1  /* v = Q * f32((double)s / N) ; W += -lr * v (sgd_quantized_gradients.py:366-371) */
#define DQRM_UPD_FP32      2  /* v = (sum_r vals_r) * (1/N); W += -lr * v   (s_q_g_p_c.py:319-327,626) */

/* Decode N gathered payloads (contiguous, payload_bytes apart), union rows, integer
 * (or rank-ordered FP32) sum, dequantize and apply SGD to W; then maintain
 * rowmax/blkmax/sblkmax/tmax and (packed != NULL && repack_bits == 4) packed rows.
 * Replaces Gloo sparse all_reduce's coalesce (s_q_g_p_c.py:878) +
 * weight_update_parallel_comm (:601-628). */
int dqrm_apply_sparse_update(const dqrm_table_set* set, const int64_t* cap_base,
                             int64_t cap_total, const void* payloads, size_t payload_bytes,
                             int num_ranks, int grad_bits, const float* s_avg, float lr,
                             int mode, int repack_bits, void* stream);

/* dqrm_apply_sparse_update with rank r's payload at payloads + r * rank_pitch
 * (rank_pitch >= payload_bytes, multiple of 16): one all-gather of several sets'
 * concatenated payloads, each set decoding its own column of the gathered buffer. */
int dqrm_apply_sparse_update_strided(const dqrm_table_set* set, const int64_t* cap_base, int64_t cap_total,
                                     const void* payloads, size_t payload_bytes, size_t rank_pitch, int num_ranks,
                                     int grad_bits, const float* s_avg, float lr, int mode, int repack_bits,
                                     void* stream);

/* dqrm_apply_sparse_update_strided on the gathered payloads, then dqrm_emb_fwd(set, next,
 * fwd_bits, fwd_flags, out, out_stride_t, out_stride_b) on the NEXT batch -- the same results as
 * those two calls (W, the |W| hierarchy, scale[] and out bit for bit). When the apply takes the
 * merge kernel (only when DQRM_APPLY_MERGE is set, at num_ranks <= 16 and <= 64 tables with the
 * workspace below; never under AUTO) and `next` is a Criteo-form batch with bags, without
 * DQRM_FWD_USE_PACKED, the forward runs in the apply's launch: each table's
 * forward workgroups start once that table's update and |W| maxima are final (no finalize or
 * forward launch). When the flat apply kernel takes it (AUTO at num_ranks < dim/4) and the
 * forward reads the exact FP32 rows, the flat kernel's finalize and the forward share ONE launch
 * after it (the forward's index and row loads in flight while the table's maxima are finalized;
 * each table's scale taken once its finalize workgroup opened the table's gate). Reference: weight_update_parallel_comm (s_q_g_p_c.py:601-628) and the next
 * apply_emb (dlrm_s_pytorch_single_gpu.py:609-674, q_m_n_q_g.py:317-398). */
int dqrm_apply_sparse_update_fwd(const dqrm_table_set* set, const int64_t* cap_base, int64_t cap_total,
                                 const void* payloads, size_t payload_bytes, size_t rank_pitch, int num_ranks,
                                 int grad_bits, const float* s_avg, float lr, int mode, int repack_bits,
                                 void* workspace, size_t workspace_bytes, const dqrm_batch* next, int fwd_bits,
                                 uint32_t fwd_flags, float* out, int64_t out_stride_t, int64_t out_stride_b,
                                 void* stream);

/* Caller workspace of the merge apply at num_ranks > 1 (the positions of every entry's row in
 * every rank's payload: num_ranks^2 * cap_total ints; 0 at one rank). dqrm_apply_sparse_update_fwd
 * with a smaller workspace (or NULL) runs the flat apply kernel. next == NULL: the apply alone. */
size_t dqrm_apply_workspace_bytes(int num_ranks, int64_t cap_total);

/* 1 if dqrm_apply_sparse_update_fwd would run the update of num_ranks payloads (with that
 * workspace) and the forward of `next` with ONE update launch, 0 if not, <0 on bad arguments. */
int dqrm_apply_fwd_is_one_launch(const dqrm_table_set* set, int num_ranks, int64_t cap_total, size_t workspace_bytes,
                                 const dqrm_batch* next, uint32_t fwd_flags);

/* The launches dqrm_apply_sparse_update_fwd would issue for these arguments: DQRM_APPLY_FWD_SEPARATE
 * (the apply's launches, then the forward's), DQRM_APPLY_FWD_ONE_LAUNCH (update and forward in one
 * launch: the merge kernel) or DQRM_APPLY_FWD_FIN_FWD (the flat apply, then its finalize and the
 * forward in one launch); <0 on bad arguments. */
#define DQRM_APPLY_FWD_SEPARATE   0
#define DQRM_APPLY_FWD_ONE_LAUNCH 1
#define DQRM_APPLY_FWD_FIN_FWD    2
int dqrm_apply_fwd_form(const dqrm_table_set* set, int num_ranks, int64_t cap_total, size_t workspace_bytes,
                        const dqrm_batch* next, uint32_t fwd_flags);

/* Single-rank DP step (num_ranks == 1, mode DQRM_UPD_DP), dqrm_grad_quant_pack and
 * dqrm_apply_sparse_update fused: the table scale s = clamp(max_s ws_absmax[t*S+s], 1e-8)
 * / (2^(bits-1)-1) (-> s_avg[t]), q = quantize(v, s) per coalesced entry, and
 * W += -lr * ((q * 1) * s) straight from the coalesce workspace, with the same rounding
 * as the payload round trip (bit-identical W, rowmax/blkmax/sblkmax/tmax, s_avg and,
 * with repack_bits == 4, packed rows). No payload is written. Replaces, at world size 1,
 * quantize_emb_grad (s_q_g_p_c.py:861-869) + weight_update_parallel_comm (:601-628). */
int dqrm_apply_local(const dqrm_table_set* set, const int64_t* ws_cap_base, int64_t ws_cap_total,
                     const int32_t* ws_rows, const float* ws_vals, const int32_t* ws_ucount,
                     const float* ws_absmax, int grad_bits, float* s_avg, float lr, int repack_bits,
                     void* stream);

/* World size 1: dqrm_emb_bwd_coalesce followed by dqrm_apply_local, with the same results
 * (W, the |W| hierarchy, s_avg, packed rows; the workspace's rows, counts and maxima -- its
 * values are scratch: a slot that fits keeps them on chip) -- for a
 * Criteo-form batch (DQRM_BATCH_POOLING_ONE, num_bags <= 4096, num_tables <= 32) in ONE
 * launch: each table's workgroups meet once to share their gradient maxima and then
 * update their row ranges, the W rows having been read during the coalesce. Replaces
 * quantize_emb_grad (s_q_g_p_c.py:850-869) + weight_update_parallel_comm (:601-628) at N=1,
 * the order grad_update_parallel_comm -> weight_update_parallel_comm runs them in
 * (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:1895-1904). Other batches: the two calls.
 * The one launch needs its grid, (T+7)/8*64 workgroups of 1024 threads, resident at once:
 * it is taken only when the current device's CUs x the occupancy query cover the grid and
 * the stream's CU mask (hipExtStreamCreateWithCUMask) enables every CU; otherwise (a CPX
 * partition, a masked stream) the two calls run. A workgroup that still waits too long (other
 * streams' kernels holding CUs) does not update its rows and flags DQRM_ERRF_STALL: the update
 * of that step is then incomplete, never computed from a partial table maximum. */
int dqrm_emb_bwd_apply_local(const dqrm_table_set* set, const dqrm_batch* batch, const float* dy,
                             int64_t dy_stride_t, int64_t dy_stride_b, int ste, const int64_t* ws_cap_base,
                             int64_t ws_cap_total, int32_t* ws_rows, float* ws_vals, int32_t* ws_ucount,
                             float* ws_absmax, int grad_bits, float* s_avg, float lr, int repack_bits,
                             void* workspace, size_t workspace_bytes, void* stream);

/* 1 if dqrm_emb_bwd_apply_local would run this batch as ONE launch on `stream` (the current
 * device), 0 if as the two calls, <0 on bad arguments. */
int dqrm_bwd_apply_local_is_one_launch(const dqrm_table_set* set, const dqrm_batch* batch, void* stream);

/* World size 1, the step boundary of a training loop: dqrm_emb_bwd_apply_local on `batch`,
 * then dqrm_emb_fwd(set, next, fwd_bits, fwd_flags, out, out_stride_t, out_stride_b) on the
 * NEXT batch -- with the same results as those two calls (W and the |W| hierarchy, s_avg,
 * scale[] and out bit for bit). In the training loop these two are adjacent: the embedding
 * backward + update of step i (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:1895-1904, at N=1)
 * and apply_emb of step i+1 (dlrm_s_pytorch_single_gpu.py:609-674, q_m_n_q_g.py:317-398),
 * whose indices the data loader has ready. When the update takes its one launch and `next`
 * is a Criteo-form batch of the same size without DQRM_FWD_USE_PACKED, the forward runs in
 * that launch: each table's workgroups, once the table's update and |W| maxima are final,
 * gather and fake-quantize the next batch's rows of that table (no second launch, no wait
 * for the other tables). Otherwise the two calls run. Error flags as the two calls'. */
int dqrm_emb_bwd_apply_fwd_local(const dqrm_table_set* set, const dqrm_batch* batch, const float* dy,
                                 int64_t dy_stride_t, int64_t dy_stride_b, int ste, const int64_t* ws_cap_base,
                                 int64_t ws_cap_total, int32_t* ws_rows, float* ws_vals, int32_t* ws_ucount,
                                 float* ws_absmax, int grad_bits, float* s_avg, float lr, int repack_bits,
                                 void* workspace, size_t workspace_bytes, const dqrm_batch* next, int fwd_bits,
                                 uint32_t fwd_flags, float* out, int64_t out_stride_t, int64_t out_stride_b,
                                 void* stream);

/* 1 if dqrm_emb_bwd_apply_fwd_local would run batch + next as ONE launch on `stream`, 0 if
 * not, <0 on bad arguments. */
int dqrm_bwd_apply_fwd_local_is_one_launch(const dqrm_table_set* set, const dqrm_batch* batch,
                                           const dqrm_batch* next, uint32_t fwd_flags, void* stream);

/* Which kernel dqrm_apply_sparse_update launches (process-wide; returns the previous
 * choice, or DQRM_E_INVALID). FLAT: one lane group per payload entry over the whole chip,
 * rows located in the other ranks' sorted row lists by binary search; SLOT: one workgroup
 * per (table, row-range slot), entries (row, rank) sorted in LDS. Both give bit-identical
 * results. AUTO (default; the environment variable DQRM_APPLY=flat|slot overrides it)
 * picks FLAT for num_ranks == 1 or num_ranks < dim/4 (one binary search per lane) and
 * SLOT above, where the per-entry searches cost more than the slot sort. */
#define DQRM_APPLY_AUTO 0
#define DQRM_APPLY_FLAT 1
#define DQRM_APPLY_SLOT 2
/* RANGES: one workgroup per block-aligned row range (a row-range slot cut in chunks) with
 * every rank's entries of it, rows owned: shrunk block maxima re-reduced in the workgroup,
 * the table's last workgroup re-reduces flagged superblocks -- no finalize launch
 * (DQRM_APPLY=ranges) */
#define DQRM_APPLY_RANGES 3
/* MERGE (opt-in, DQRM_APPLY=merge; <= 16 ranks, <= 64 tables; N > 1 needs the positions
 * workspace of dqrm_apply_sparse_update_fwd): k_merge_pos locates every entry's row in the other
 * ranks' payloads in LDS per block-aligned row range, k_apply_pos updates one lane group per entry
 * with the positions read in one load and finalizes the hierarchy in-launch; with a next batch its
 * forward runs in that launch behind per-table gates. Bit-exact with FLAT; not faster on the TB
 * shape, hence not AUTO. */
#define DQRM_APPLY_MERGE 4
int dqrm_set_apply_kernel(int kind);

/* Which backward kernels dqrm_emb_bwd_coalesce and dqrm_emb_bwd_sgd launch (process-wide;
 * returns the previous choice, or DQRM_E_INVALID). AUTO (default): batches in the Criteo
 * form (DQRM_BATCH_POOLING_ONE) with num_bags <= 4096 and max_lookups >= num_bags take the
 * Criteo-form coalesce kernel (dqrm_coalesce.hip), and SGD batches of at most 512 lookups
 * per table (fewer for D > 32) with num_bags * dim <= 16384 the one-workgroup-per-table SGD
 * kernel; everything else the general (sorting) kernel. GENERAL: always the general
 * kernel. Both give bit-identical results (coalesce: rows, values, counts, the max over a
 * table's DQRM_TABLE_SPLIT ws_absmax entries; SGD: W, the |W| maxima, packed rows). */
#define DQRM_COALESCE_AUTO 0
#define DQRM_COALESCE_GENERAL 1
int dqrm_set_coalesce_kernel(int kind);

/* ---------------------------------------------------------------------------------
 * Dense (MLP) layer gradients, data-parallel:
 *   quantize_linear_grad (per-channel) / quantize_bias_grad   s_q_g_p_c.py:892-961
 *   MLP branch of grad_update_parallel_comm                   s_q_g_p_c.py:337-409
 *   MLP branch of weight_update_parallel_comm                 s_q_g_p_c.py:630-668
 * A dense set is C "channels" over the bot_l/top_l Linear layers: every weight row is a
 * channel (per_channel=True, one scale per output feature) and every bias vector is one
 * channel (one scale per bias). Channel c is len[c] contiguous floats at grad[c] (the
 * layer's .grad) and param[c] (the layer's .data); its quantized values sit at
 * [wire_off[c], +len[c]) of the wire buffer. The arrays are device arrays.
 * Per step: scale -> all-gather of s_loc [C] -> quant -> all-reduce(SUM) of the wire ->
 * decode (grad_update_parallel_comm) ; update (weight_update_parallel_comm).
 * ------------------------------------------------------------------------------ */
typedef struct dqrm_dense_set {
    int32_t  num_channels;    /* C */
    int32_t  max_len;         /* max_c len[c] (host-side hint) */
    int64_t  total_elems;     /* wire elements = sum_c len[c] */
    float* const*  grad;      /* [C] device pointers to each channel's gradient */
    float* const*  param;     /* [C] device pointers to each channel's parameter */
    const int32_t* len;       /* [C] */
    const int64_t* wire_off;  /* [C] element offset of the channel in the wire */
} dqrm_dense_set;

/* wire element types of the quantized-gradient all-reduce */
#define DQRM_WIRE_F16 1  /* integer-valued fp16: exact sums for bits <= 8 and N <= 16 (|sum| <= 2048) */
#define DQRM_WIRE_I32 2  /* int32: exact for bits <= 16 */
#define DQRM_WIRE_F32 3  /* unquantized FP32 gradients (mlp_layer_quantized=False, :358-369) */

/* Host helper: the narrowest exact wire type for (bits, num_ranks); bits == 32 -> F32;
 * <0 if unsupported. */
int dqrm_dense_wire_type(int bits, int num_ranks);

/* Local per-channel scale (:905-912, quant_utils.py:196-220):
 *   s_loc[c] = clamp(max(|min_j g|, |max_j g|), 1e-8) / (2^(bits-1)-1). */
int dqrm_dense_grad_scale(const dqrm_dense_set* set, int bits, float* s_loc, void* stream);

/* Scale average + quantize into the wire (:913-918 / :945-950). s_all = the N ranks'
 * s_loc gathered [N][C]:
 *   s_avg[c] = (((s_{N-1} + s_{N-2}) + ...) + s_0) * (1/N)   (same order on every rank)
 *   wire     = clamp(round(1/s_avg[c] * g + 0), -2^(bits-1), 2^(bits-1)-1)
 * wire_type F32 copies the gradient unquantized (s_all, s_avg unused, may be NULL). */
int dqrm_dense_grad_quant(const dqrm_dense_set* set, int bits, const float* s_all, int num_ranks,
                          float* s_avg, int wire_type, void* wire, void* stream);

/* After the wire's all-reduce(SUM): grad = 0 + wire * (1/N)  (:920-922 then the hook's
 * grad.zero_(); grad.add_(buffer_changes), :345-351). */
int dqrm_dense_grad_decode(const dqrm_dense_set* set, const void* wire, int wire_type, int num_ranks,
                           void* stream);

/* weight_update_parallel_comm, MLP branch (:641-642 / :659-660):
 *   param += (-lr * grad) * s[c]     (s == NULL: param += -lr * grad, :644-645). */
int dqrm_dense_update(const dqrm_dense_set* set, const float* s, float lr, void* stream);

/* Simulated DP (one device plays N ranks, sgd_quantized_gradients.py): the MLP half of
 * grad_buffer_update_added_quantization (:96-139) with the error compensation of
 * quantize_linear_grad / quantize_bias_grad (:563-632, err_compensation=True, per channel).
 * One micro-step, ONE launch for all channels; scale [C], err and buf [total_elems] laid out by
 * wire_off, every operation a separately rounded f32 one:
 *   v = grad + err
 *   scale[c] == 0 (first micro-step since zeroing):
 *       scale[c] = clamp(max_j |v_j|, 1e-8) / (2^(bits-1)-1)      (quant_utils.py:196-220)
 *   q   = clamp(round(1/scale[c] * v + 0), -2^(bits-1), 2^(bits-1)-1)   (quant_utils.py:75-101, 316-346)
 *   buf = buf + q
 *   err = v - q * scale[c]
 * A scale once set is >= 1e-8/qmax > 0, so scale[c] == 0 is the reference's host-side
 * "sum of the tensor's scales is zero" test with no host read. Zeroing (:261-308) is the
 * caller's: buf = 0 and scale = 0; err carries over. bits 2..16 (the reference hard-codes 8). */
int dqrm_dense_ec_accumulate(const dqrm_dense_set* set, int bits, float* scale, float* err, float* buf,
                             void* stream);

/* weights_update_added_quantization, MLP branch (:381-404), ONE launch:
 *   param = param + (-lr) * (buf * (scale[c] / num_gpus))    (scale / N a true f32 division) */
int dqrm_dense_sim_update(const dqrm_dense_set* set, const float* scale, const float* buf, int num_gpus,
                          float lr, void* stream);

/* ---------------------------------------------------------------------------------
 * QuantLinear: the fake-quantized MLP layer (quantization_supp/
 * quant_modules_not_quantize_grad.py:20-211), csrc/dqrm_linear.hip.
 * Every `*`, `/` and `+` below is one separately rounded f32 operation, and every sum is the
 * chain  acc = 0; acc = fmaf(a_k, b_k, acc)  in ascending k (one rounding per product), which
 * is what v_mfma_f32_16x16x4_f32 computes: the bits are a function of the operands and the
 * shapes alone (no atomics, no split reductions, the same for every batch slice a row is in).
 * weight_integer / bias_integer hold integer values as f32, as the reference keeps them.
 * scale is [out_features] with per_channel, [1] otherwise. All pointers are device pointers.
 * ------------------------------------------------------------------------------ */
typedef struct dqrm_linear {
    int32_t in_features;      /* K */
    int32_t out_features;     /* O */
    int32_t weight_bit;       /* 2..32 (quantized calls only) */
    int32_t bias_bit;         /* 2..32 (quantized calls only) */
    int32_t per_channel;      /* one scale per output feature / one for the tensor */
    int32_t reserved;
    const float* weight;      /* [O][K] */
    const float* bias;        /* [O] */
    float* weight_integer;    /* [O][K] */
    float* bias_integer;      /* [O] */
    float* scale;             /* [O] or [1]: fc_scaling_factor */
} dqrm_linear;

/* The quantization half of QuantLinear.forward (q_m_n_q_g.py:121-154):
 *   n = 2^(weight_bit-1) - 1, nb = 2^(bias_bit-1) - 1
 *   scale[o] = clamp(max(|min_k W[o,k]|, |max_k W[o,k]|), 1e-8) / n      (quant_utils.py:196-220;
 *              per_channel == 0: one scale over the whole tensor)
 *   weight_integer = clamp(round(1/scale * W + 0), -n-1, n)               (quant_utils.py:75-101,329-346)
 *   bias_integer   = clamp(round(1/scale[o] * b[o] + 0), -nb-1, nb)       (the WEIGHT's scale, :150-154)
 * One launch with per_channel, two without. */
int dqrm_linear_wquant(const dqrm_linear* layer, void* stream);

/* QuantLinear.forward's product (q_m_n_q_g.py:209 / :211), x [B][K] -> y [B][O]:
 *   acc = chain over k of x[b,k] * weight_integer[o,k]
 *   quantized:      y[b,o] = (acc + bias_integer[o]) * scale[o]   (F.linear(...) * fc_scaling_factor)
 *   not quantized:  the operands are weight and bias, y[b,o] = acc + bias[o]  (full_precision_flag)
 * One launch. */
int dqrm_linear_fwd(const dqrm_linear* layer, int quantized, const float* x, int64_t B, float* y, void* stream);

/* Backward of the above through the straight-through estimator (quant_utils.py:349-363: the
 * gradient of weight_integer / bias_integer is divided by the scale), g[b,o] = dy[b,o] * scale[o]:
 *   dx[b,k] = chain over o of g[b,o] * weight_integer[o,k]          (dx == NULL: skipped)
 *   dw[o,k] = (chain over b of g[b,o] * x[b,k]) / scale[o]
 *   db[o]   = (chain over b of g[b,o]) / scale[o]
 * not quantized: scale = 1, the operand is weight, no division. Two launches (db rides in the dw
 * kernel), one when dx == NULL. */
int dqrm_linear_bwd(const dqrm_linear* layer, int quantized, const float* x, const float* dy, int64_t B,
                    float* dx, float* dw, float* db, void* stream);

/* The activation create_mlp puts after every layer (dlrm_s_pytorch_comm_grad.py:279-343: nn.ReLU,
 * nn.Sigmoid after the last), fused into the layer's kernels. Let z[b,o] be exactly what
 * dqrm_linear_fwd produces (chain, bias and scale included); every operation named is one
 * separately rounded f32 operation:
 *
 *   act               forward y[b,o]                   backward d[b,o]
 *   DQRM_ACT_NONE     z                                dy
 *   DQRM_ACT_RELU     z <= 0 ? 0 : z                   y <= 0 ? 0 : dy
 *   DQRM_ACT_SIGMOID  1.0f / (1.0f + expf(-z))         (dy * (1.0f - y)) * y
 *
 * RELU keeps a NaN and turns -0 into +0; its backward is torch's threshold_backward on the
 * result. SIGMOID's backward is torch's sigmoid_backward in its order of operations.
 * d replaces dy in dqrm_linear_bwd's formulas: g[b,o] = d[b,o] * scale[o], and dx, dw and db are
 * the unchanged chains over g (dx == NULL: skipped). y is the forward's output [B][O], read with
 * dy's addressing: required when act != DQRM_ACT_NONE, ignored (may be NULL) when it is.
 * DQRM_E_INVALID before any device work: act outside 0..2, act != NONE with y == NULL in the
 * backward, and everything dqrm_linear_fwd / _bwd reject. With DQRM_ACT_NONE the calls are
 * dqrm_linear_fwd / _bwd bit for bit. The launch counts do not change: forward one, backward
 * two, one when dx == NULL. */
enum { DQRM_ACT_NONE = 0, DQRM_ACT_RELU = 1, DQRM_ACT_SIGMOID = 2 };

int dqrm_linear_fwd_act(const dqrm_linear* layer, int quantized, int act,
                        const float* x, int64_t B, float* y, void* stream);
int dqrm_linear_bwd_act(const dqrm_linear* layer, int quantized, int act,
                        const float* x, const float* y, const float* dy, int64_t B,
                        float* dx, float* dw, float* db, void* stream);

/* QuantLinear's integer-activation branch (quantize_activation with a prev_act_scaling_factor,
 * q_m_n_q_g.py:150-161, :193-196), on the same kernels as the calls above and under the same
 * arithmetic rules. Two more device pointers:
 *   prev       one float, p: the previous activation scale (QuantAct's act_scaling_factor, or the
 *              out_scale of the layer before)
 *   out_scale  [O] with per_channel, [1] otherwise: cos[o] = scale[o] * p, the reference's
 *              bias_scaling_factor / correct_output_scale
 * p has ONE element. A per-channel cos of layer i cannot be the prev of layer i+1: the reference
 * breaks there too (`fc_scaling_factor.view(1,-1) * prev.view(1,-1)` does not broadcast [1,O']
 * against [1,O]). Quantized only; there is no full-precision form.
 *
 * dqrm_linear_wquant_qact: scale and weight_integer as dqrm_linear_wquant writes them, bit for
 * bit, and
 *   out_scale[o]    = scale[o] * p
 *   bias_integer[o] = clamp(round(1/out_scale[o] * b[o] + 0), -nb-1, nb)            (:150-154)
 * One launch with per_channel, two without.
 *
 * dqrm_linear_fwd_qact, x [B][K] -> y [B][O], one launch:
 *   acc    = chain over k of (x[b,k] / p) * weight_integer[o,k]     (x / p formed on load, :160)
 *   y[b,o] = act(rintf(acc + bias_integer[o]) * cos[o])             (ste_round(F.linear) * cos, :194-196)
 * with act as in dqrm_linear_fwd_act.
 *
 * dqrm_linear_bwd_qact, d = dy * act'(y) as in dqrm_linear_bwd_act, g[b,o] = d[b,o] * cos[o]
 * (ste_round passes g through):
 *   dx[b,k] = (chain over o of g[b,o] * weight_integer[o,k]) / p     (dx == NULL: skipped)
 *   dw[o,k] = (chain over b of g[b,o] * (x[b,k] / p)) / scale[o]
 *   db[o]   = (chain over b of g[b,o]) / cos[o]
 * Two launches, one when dx == NULL.
 *
 * DQRM_E_INVALID before any device work: everything dqrm_linear_wquant / _fwd_act / _bwd_act
 * reject for a quantized layer, and a null prev / out_scale. B == 0 in the forward: DQRM_OK, no
 * launch. */
int dqrm_linear_wquant_qact(const dqrm_linear* layer, const float* prev, float* out_scale, void* stream);
int dqrm_linear_fwd_qact(const dqrm_linear* layer, int act, const float* x, const float* prev,
                         const float* out_scale, int64_t B, float* y, void* stream);
int dqrm_linear_bwd_qact(const dqrm_linear* layer, int act, const float* x, const float* y, const float* dy,
                         const float* prev, const float* out_scale, int64_t B,
                         float* dx, float* dw, float* db, void* stream);

/* ---------------------------------------------------------------------------------
 * A whole MLP stack (create_mlp's QuantLinear layers with their fused activations) per host
 * call, csrc/dqrm_mlp.hip. The struct and its three arrays are HOST memory; the pointers inside
 * each dqrm_linear, and the entries of every pointer array below, are device pointers.
 * dqrm_mlp_fwd / _bwd run weight-only layers; dqrm_mlp_fwd_qact / _bwd_qact below are their
 * integer-activation (quantize_activation) forms.
 * ------------------------------------------------------------------------------ */
#define DQRM_MLP_MAX_LAYERS 16   /* the update kernel takes the layer descriptors by value */
typedef struct dqrm_mlp {
    int32_t num_layers;           /* L, 1..DQRM_MLP_MAX_LAYERS */
    int32_t reserved;
    const dqrm_linear* layers;    /* HOST [L]; layers[i].in_features == layers[i-1].out_features */
    const int32_t* quantized;     /* HOST [L]: 0 = full_precision_flag */
    const int32_t* act;           /* HOST [L]: DQRM_ACT_* fused into layer i */
} dqrm_mlp;

#define DQRM_MLP_FRESH   1u   /* fwd: integers and scales are current, launch no wquant */
#define DQRM_MLP_REQUANT 1u   /* sgd: refresh scale / weight_integer / bias_integer of quantized layers */

/* The stack's forward: for layer i = 0..L-1, dqrm_linear_wquant (quantized layers, unless
 * DQRM_MLP_FRESH) and dqrm_linear_fwd_act with x_i = x or y[i-1], by calling those exports, in
 * that order: the per-layer calls' launches and bits. y is a HOST array of L device pointers,
 * y[i] is [B][out_i]; every y[i] is also what the backward reads. L launches, plus the wquant
 * launches when not fresh. B == 0: DQRM_OK, no launch. */
int dqrm_mlp_fwd(const dqrm_mlp* stack, uint32_t flags, const float* x, int64_t B, float* const* y, void* stream);

/* The stack's backward: dqrm_linear_bwd_act from layer L-1 to layer 0; layer i's dx is written to
 * one of two scratch buffers of [B][max hidden width] floats and is layer i-1's dy; layer 0's goes
 * to dx (NULL: skipped). dw / db are HOST arrays of L device pointers. The scratch is
 * dqrm_mlp_bwd_scratch_bytes = 2 * B * (max over i < L-1 of out_i) * 4 bytes (0 for one layer).
 * 2L - 1 launches, 2L with dx. */
size_t dqrm_mlp_bwd_scratch_bytes(const dqrm_mlp* stack, int64_t B);
int dqrm_mlp_bwd(const dqrm_mlp* stack, const float* x, const float* const* y, const float* dy, int64_t B,
                 float* dx, float* const* dw, float* const* db, void* scratch, size_t scratch_bytes, void* stream);

/* SGD on every layer of the stack, and (DQRM_MLP_REQUANT) the quantization the next forward
 * needs, so that it can run DQRM_MLP_FRESH. weight / bias of the layers are WRITTEN (the struct's
 * const is dqrm_linear's). Every product and sum is one separately rounded f32 operation:
 *   nlr = -lr
 *   W[o,k] = W[o,k] + (nlr * dw[o,k])                      gscale == NULL  (s_q_g_p_c.py:645-646)
 *   W[o,k] = W[o,k] + ((nlr * dw[o,k]) * gscale[l][o])     gscale given    (:642-643, dqrm_dense_update)
 *   b[o]   = b[o]   + (nlr * db[o])  [ * gscale[l][out_l] ]
 * gscale: HOST array of L device pointers, gscale[l] is [out_l + 1]: the rows' scales, then the
 * bias's. With DQRM_MLP_REQUANT a quantized layer's scale, weight_integer and bias_integer
 * afterwards hold exactly what dqrm_linear_wquant writes from the updated W and b; full-precision
 * layers are updated only. One launch; two when DQRM_MLP_REQUANT meets a quantized layer without
 * per_channel, whose row maxima pass through the workspace (dqrm_mlp_sgd_workspace_bytes: 4 bytes
 * per weight row of the stack, 0 when no quantized layer is per tensor). No atomics, no memset,
 * nothing that depends on workgroups being resident together.
 *
 * All five calls: DQRM_E_INVALID before any launch for a null stack or array, num_layers outside
 * 1..DQRM_MLP_MAX_LAYERS, a width chain that does not match, act outside 0..2, what
 * dqrm_linear_wquant / _fwd / _bwd reject in a layer, unknown flags, a null x / dy or entry of
 * y / dw / db / gscale, a short scratch or workspace, B < 0 (B < 1 in the backward). The two size
 * queries return 0 for a stack they reject. */
size_t dqrm_mlp_sgd_workspace_bytes(const dqrm_mlp* stack);
int dqrm_mlp_sgd(const dqrm_mlp* stack, uint32_t flags, const float* const* dw, const float* const* db,
                 const float* const* gscale, float lr, void* workspace, size_t workspace_bytes, void* stream);

/* dqrm_mlp_sgd on several stacks (a model's bottom and top MLP) in ONE launch: the same kernels
 * over the rows of all the stacks' layers, so per (layer, row) the same formulas, roundings and
 * bits as dqrm_mlp_sgd on each stack alone. stacks: HOST array of num_stacks stacks, each checked
 * as dqrm_mlp_sgd checks it (its own width chain included); their layers number at most
 * DQRM_MLP_MAX_LAYERS in all. dw / db / gscale: HOST arrays over the layers of stacks[0], then
 * stacks[1], ... Two launches when DQRM_MLP_REQUANT meets a quantized per-tensor layer in any of
 * them; the workspace is then 4 bytes per weight row of ALL the stacks
 * (dqrm_mlp_sgd_multi_workspace_bytes; 0 otherwise, and 0 for arguments it rejects). */
size_t dqrm_mlp_sgd_multi_workspace_bytes(const dqrm_mlp* const* stacks, int num_stacks);
int dqrm_mlp_sgd_multi(const dqrm_mlp* const* stacks, int num_stacks, uint32_t flags, const float* const* dw,
                       const float* const* db, const float* const* gscale, float lr, void* workspace,
                       size_t workspace_bytes, void* stream);

/* The integer-activation (quantize_activation) stack: every layer runs dqrm_linear_*_qact, layer
 * i's prev being `prev` (one float, the QuantAct's scale in front of the stack) for i == 0 and
 * out_scale[i-1] otherwise. out_scale: HOST array of L device pointers, out_scale[i] is [1], or
 * [out_i] for a per-channel layer; the forward WRITES them and the backward reads them.
 *
 * dqrm_mlp_qact_prepare, ONE launch for all layers: the half of dqrm_linear_wquant_qact that
 * depends on the activation scale. With p_0 = prev[0] and p_(i+1) = scale_i[0] * p_i:
 *   out_scale_i[o]    = scale_i[o] * p_i             (scale_i[0] without per_channel)
 *   bias_integer_i[o] = clamp(rintf(1 / out_scale_i[o] * b_i[o] + 0))     to bias_bit
 * each a separately rounded f32 operation: bit for bit what L calls of dqrm_linear_wquant_qact
 * leave in out_scale and bias_integer. It READS the layers' scale, so it is valid only while
 * scale and weight_integer are current (dqrm_mlp_sgd with DQRM_MLP_REQUANT, or a wquant, since the
 * last write to the weights). No atomics, no workgroup waits on another.
 *
 * dqrm_mlp_fwd_qact: with DQRM_MLP_FRESH one prepare launch, then dqrm_linear_fwd_qact per layer
 * (L + 1 launches); without it dqrm_linear_wquant_qact and dqrm_linear_fwd_qact per layer. B == 0:
 * the out_scales and bias integers are still written, no GEMM runs.
 * dqrm_mlp_bwd_qact: dqrm_linear_bwd_qact from layer L-1 to layer 0 with dqrm_mlp_bwd's two
 * scratch buffers (dqrm_mlp_bwd_scratch_bytes) and launch counts.
 *
 * dqrm_mlp_sgd and _multi are unchanged: with DQRM_MLP_REQUANT they write bias_integer with the
 * WEIGHT's scale, which is not what an integer-activation layer reads; the next forward's prepare
 * (or wquant_qact) overwrites it before any GEMM does. scale and weight_integer are what they
 * keep current for such a stack.
 *
 * DQRM_E_INVALID before any launch: everything dqrm_mlp_fwd / _bwd reject; a layer with
 * quantized[i] == 0 (the reference's scale chain breaks there); per_channel on any layer but the
 * last (an [out] out_scale cannot be the next layer's one-element prev); a null prev, out_scale
 * array or entry. */
int dqrm_mlp_qact_prepare(const dqrm_mlp* stack, const float* prev, float* const* out_scale, void* stream);
int dqrm_mlp_fwd_qact(const dqrm_mlp* stack, uint32_t flags, const float* x, const float* prev,
                      float* const* out_scale, int64_t B, float* const* y, void* stream);
int dqrm_mlp_bwd_qact(const dqrm_mlp* stack, const float* x, const float* const* y, const float* dy,
                      const float* prev, float* const* out_scale, int64_t B, float* dx, float* const* dw,
                      float* const* db, void* scratch, size_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * QuantAct: fake-quantized activations with a running range (quantization_supp/
 * quant_modules_not_quantize_grad.py:541-725), csrc/dqrm_act.hip. Symmetric, one scale for the
 * tensor, act_percentile == 0. Every `*`, `/` and `+` below is one separately rounded f32
 * operation; min and max are exact and order-independent; nothing is read back to the host (the
 * reference's `if self.x_min == self.x_max` is taken on the device). x finite.
 *
 * dqrm_act_quant_fwd, x [numel] -> y [numel]:
 *   running_stat != 0 (QuantAct.forward:653-678), bmin = min(x), bmax = max(x):
 *     x_min == x_max:   x_min = x_min + bmin;  x_max = x_max + bmax      (an add, as written there)
 *     momentum == -1:   x_min = min(x_min, bmin);  x_max = max(x_max, bmax)
 *     otherwise:        x_min = x_min * momentum + bmin * one_minus_momentum;  x_max likewise
 *   n = 2^(activation_bit-1) - 1
 *   scale[0] = max(max(|x_min|, |x_max|), 1e-8) / n                      (quant_utils.py:196-220)
 *   y = clamp(rintf(1/scale * x + 0), -n-1, n) * scale          (quant_utils.py:101, :343; :694, :722-723)
 * y == NULL with running_stat: the range update alone (full_precision_flag), scale untouched.
 * Launches: at most THREE. With running_stat, numel > 16384: per-workgroup min / max into the
 * workspace, then one workgroup that reduces them and updates the range, then the elementwise
 * pass (3); numel <= 16384: the one workgroup reads x itself (2); without running_stat: the
 * elementwise pass alone (1). The range update is a launch of a single workgroup between the
 * other two, so no workgroup reads a half-updated range.
 * workspace: dqrm_act_quant_workspace_bytes(numel) bytes of device memory, 4-byte aligned, contents
 * irrelevant; may be NULL when that is 0 or running_stat is 0.
 *
 * dqrm_act_quant_bwd: dx = (dy * scale[0]) / scale[0]  (quant_utils.py:349-363 under the
 * `* correct_output_scale` of :723), one launch; a caller whose input needs no gradient does
 * not call it.
 *
 * DQRM_E_INVALID before any device work: a null struct, activation_bit outside 2..32, null
 * x_min / x_max / scale, negative numel, null x (or y without running_stat), a null workspace
 * where one is needed; null scale / dy / dx in the backward. numel == 0: DQRM_OK, no launch, the
 * range left alone.
 * ------------------------------------------------------------------------------ */
typedef struct dqrm_act_quant {
    int32_t activation_bit;    /* 2..32 */
    int32_t running_stat;      /* update x_min / x_max from this batch */
    float momentum;            /* act_range_momentum; -1: running min / max */
    float one_minus_momentum;  /* (float)(1.0 - (double)act_range_momentum): what torch multiplies an
                                  f32 tensor with for the Python scalar `1 - momentum` */
    float* x_min;              /* [1] */
    float* x_max;              /* [1] */
    float* scale;              /* [1]: act_scaling_factor */
} dqrm_act_quant;

int64_t dqrm_act_quant_workspace_bytes(int64_t numel);
int dqrm_act_quant_fwd(const dqrm_act_quant* q, const float* x, int64_t numel, float* y, void* workspace,
                       void* stream);
int dqrm_act_quant_bwd(const float* scale, const float* dy, int64_t numel, float* dx, void* stream);

/* ---------------------------------------------------------------------------------
 * DLRMLoss: the model's head, csrc/dqrm_loss.hip. DLRM_Net.forward's
 * `torch.clamp(p, min=loss_threshold, max=1.0 - loss_threshold)`
 * (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:837-839, :877-879) and loss_fn_wrap (:193-212):
 * BCELoss / MSELoss(reduction="mean"), or for "wbce" loss_ws[T.long()] * BCELoss(reduction="none")
 * and .mean(). All f32, every operation below rounded on its own, nothing read back to the host.
 *
 * Per sample, p the top MLP's output and t the target (B contiguous floats each):
 *   z = clamp ? min(max(p, lo), hi) : p            NaN propagating (a caller passes
 *       lo = (float)loss_threshold, hi = (float)(1.0 - (double)loss_threshold): what torch.clamp
 *       compares an f32 tensor with for those Python scalars; clamp only if 0 < threshold < 1)
 *   DQRM_LOSS_BCE   l = (t - 1) * max(log1pf(-z), -100) - t * max(logf(z), -100)      w = 1
 *                   d = (z - t) / max((1 - z) * z, 1e-12f)
 *   DQRM_LOSS_MSE   l = (z - t) * (z - t)           d = 2 * (z - t)                       w = 1
 *   DQRM_LOSS_WBCE  BCE's l and d, w = weights[(int64)t]; a class outside [0, num_weights) reads
 *                   no memory: w = NaN, so that sample's term and gradient and the loss are NaN.
 *                   (The reference keeps loss_ws in float64 and its wbce loss is float64; here
 *                   the weights are f32 and so is the loss.)
 *   Both max() keep a NaN. z outside [0, 1] is outside BCELoss's domain (torch asserts): NaN here.
 *   terms[i] = w * l
 *   g[i]     = (w * d) / (float)B;  0 where the clamp cut (p < lo or p > hi: torch's bounds are
 *              inclusive); a NaN p gives NaN
 *   loss[0]  = S / (float)B, S the sum of the terms in an order that is a function of B alone:
 *              slot s = i mod 256 starts at +0.0f and adds its terms i = s, s + 256, ... in
 *              ascending i; the slots are folded with slot[s] += slot[s + stride] for
 *              stride = 128, 64, ..., 1; S = slot[0]. Plain f32 adds. The bits of the loss do
 *              not depend on the grid, the device or the stream.
 * dqrm_loss_fwd is exactly ONE launch (one workgroup of 256 threads, thread s owning slot s) and
 * no memset: the kernel writes loss[0] itself. g NULL: an inference-only loss. z (the clamped
 * prediction, DLRM_Net.forward's return value) and terms (reduction="none") may be NULL.
 *
 * dqrm_loss_bwd: dp = go[0] * g, one launch; go is the 0-dim upstream gradient in device memory.
 * A caller whose p needs no gradient does not call it.
 *
 * DQRM_E_INVALID before any device work: a null struct, an unknown kind, DQRM_LOSS_WBCE without
 * weights (NULL or num_weights < 1), B < 1 or B > 2^20 (the one-workgroup forward's limit),
 * null p / t / loss; null g / go / dp in the backward.
 * ------------------------------------------------------------------------------ */
enum { DQRM_LOSS_BCE = 0, DQRM_LOSS_MSE = 1, DQRM_LOSS_WBCE = 2 };

typedef struct dqrm_loss {
    int32_t kind;          /* DQRM_LOSS_BCE / _MSE / _WBCE */
    int32_t clamp;         /* 0 / 1 */
    float lo, hi;          /* the clamp's bounds (ignored when clamp == 0) */
    int32_t num_weights;   /* wbce: entries of weights */
    const float* weights;  /* device [num_weights], wbce (ignored otherwise) */
} dqrm_loss;

int dqrm_loss_fwd(const dqrm_loss* cfg, const float* p, const float* t, int64_t B,
                  float* loss /*[1]*/, float* g /*[B], nullable*/,
                  float* z /*[B], nullable*/, float* terms /*[B], nullable*/,
                  void* stream);
int dqrm_loss_bwd(const float* g, const float* go, int64_t B, float* dp, void* stream);

/* ---------------------------------------------------------------------------------
 * DotInteraction: DLRM_Net.interact_features, arch_interaction_op "dot"
 * (dlrm_s_pytorch_comm_grad.py:701-806), csrc/dqrm_interact.hip.
 * A sample has F = num_features vectors of dim D: T[b,0,:] = x[b,:] (the bottom MLP's output) and
 * T[b,f,:] = emb[b*emb_stride_b + (f-1)*emb_stride_f + :] (the embedding outputs, read in place:
 * a [B][F-1][D] slab has strides ((F-1)*D, D), a [F-1][B][D] slab (D, B*D)). Pairs are ordered as
 * the reference's li / lj lists: for i in 0..F-1, for j in 0..i-1 (0..i with self_interaction),
 * index p(i,j) in that order; P = F(F-1)/2 (+ F). The output is r [B][D + P].
 * Every sum is the chain  acc = 0; acc = fmaf(a, b, acc)  in ascending index, one rounding per
 * product, no atomics, no split reductions; every other `*`, `/`, `+` is one separately rounded
 * f32 operation. In plain mode a sample's bits depend on that sample's operands alone.
 *
 * plain (quant_bits == 0):
 *   r[b, 0:D]        = x[b, :]                                   (a bit copy)
 *   r[b, D + p(i,j)] = chain over k of T[b,i,k] * T[b,j,k]
 *   backward, g(i,j) = dr[b, D + p(i,j)]:
 *     c(i,j) = g(i,j) for j < i, g(j,i) for j > i, g(i,i) + g(i,i) for j == i with
 *              self_interaction (without it the j == i term is absent)
 *     dT[b,i,k] = chain over j = 0..F-1 of c(i,j) * T[b,j,k]
 *     dx[b,k] = dr[b,k] + dT[b,0,k];  demb[b,f-1,k] = dT[b,f,k]   (demb contiguous [B][F-1][D])
 * quantized (quant_bits = 2..16; the reference hard-codes 16), n = 2^(bits-1) - 1:
 *   s  = clamp(max over the whole batch of |T|, 1e-8) / n        (quant_utils.py:196-220)
 *   Ti = clamp(round_half_even(1/s * T + 0), -n-1, n)            (quant_utils.py:75-101, :329-346)
 *   r[b, D + p(i,j)] = (chain over k of Ti[i,k] * Ti[j,k]) * (s * s);  r[b, 0:D] = x[b, :]
 *   backward: g(i,j) = dr[b, D + p(i,j)] * (s * s), the same c and chain over Ti, then
 *     dT = chain / s  (the STE, quant_utils.py:349-363),  dx = dr[b, 0:D] + dT[b,0]
 *
 * Argument rules (checked before any device call): 2 <= F <= 64; D a multiple of 4 in 4..256;
 * quant_bits 0 or 2..16; strides non-negative multiples of 4; pointers 16-byte aligned (scale:
 * 4-byte); B >= 0 (B == 0: DQRM_OK, no launch) and B * F * D / 4 < 2^31 (DQRM_E_CAPACITY);
 * scale non-NULL exactly when quant_bits != 0. No call allocates, synchronises or reads back:
 * the step can be captured in a HIP graph.
 * ------------------------------------------------------------------------------ */
typedef struct dqrm_interact {
    int32_t num_features;      /* F = tables + 1 */
    int32_t dim;               /* D */
    int32_t self_interaction;  /* arch_interaction_itself */
    int32_t quant_bits;        /* 0: plain; 2..16: the fake-quantized product */
    int64_t emb_stride_b;      /* elements between two samples of emb */
    int64_t emb_stride_f;      /* elements between two features of emb (the inner stride is 1) */
} dqrm_interact;

/* D + P, or a negative value for arguments outside the rules above. */
int64_t dqrm_interact_out_features(int32_t num_features, int32_t dim, int32_t self_interaction);

/* Quantized mode only: scale[0] = s on the device. A 4-byte memset and one launch, no host read. */
int dqrm_interact_scale(const dqrm_interact* cfg, const float* x, const float* emb, int64_t B, float* scale,
                        void* stream);

/* r [B][D + P]. One launch. scale: the device word dqrm_interact_scale wrote (NULL in plain mode). */
int dqrm_interact_fwd(const dqrm_interact* cfg, const float* x, const float* emb, int64_t B, const float* scale,
                      float* r, void* stream);

/* dx [B][D] and demb [B][F-1][D] from dr [B][D + P]; either may be NULL (not computed; both NULL:
 * no launch). One launch. scale: the one the forward used. */
int dqrm_interact_bwd(const dqrm_interact* cfg, const float* x, const float* emb, const float* dr, int64_t B,
                      const float* scale, float* dx, float* demb, void* stream);

/* ---------------------------------------------------------------------------------
 * DQRMNet: the whole DLRM (DLRM_Net.forward, dlrm_s_pytorch_tb_dp_one_parallel_comm.py:805-880,
 * and one iteration of its training loop at world size 1) per host call, csrc/dqrm_model.hip.
 * dqrm_model_fwd and dqrm_model_step contain no arithmetic: they validate the whole call and then
 * call the exports above in the order a stage-by-stage caller would, so every buffer they write
 * holds what that chain of calls writes, bit for bit. What they save is the host's work per stage.
 *
 * The struct is HOST memory; `tables`, `bottom`, `top` and `loss` point to host structs as the
 * stage calls take them. interact.num_features must be tables->num_tables + 1 and interact.dim
 * tables->dim; interact.emb_stride_b / _f are ignored (the library reads the embedding slab it lays
 * out itself, [B][T][D]). bottom's last width must be D, top's first
 * dqrm_interact_out_features(T + 1, D, self_interaction), top's last 1. bottom and top have at most
 * DQRM_MLP_MAX_LAYERS layers together (their update is one dqrm_mlp_sgd_multi).
 *
 * Memory: nothing is allocated. The caller passes one device workspace (16-byte aligned, contents
 * irrelevant) of dqrm_model_workspace_bytes(model, B, max_lookups) bytes, which the library cuts
 * into: the embedding slab [B][T][D] (offset 0), every layer's output, r and dr [B][D + P], dx
 * [B][D], demb [B][T][D], the MLP backward scratch, the embedding backward's sort workspace
 * (dqrm_bwd_workspace_bytes), the interaction's scale word and the per-tensor layers' row maxima.
 * The cut depends on (B, batch->max_lookups) alone and the size grows with both, so one buffer
 * sized for the largest batch serves every smaller one. dqrm_model_workspace_layout tells where
 * the slab, r, p (the top stack's output [B]), dr, dx and demb sit (byte offsets).
 *
 * dqrm_model_fwd (inference): dqrm_emb_fwd into the slab; dqrm_mlp_fwd(bottom, x);
 * dqrm_interact_scale (quant_bits != 0) and dqrm_interact_fwd; dqrm_mlp_fwd(top); and, labels
 * given, dqrm_loss_fwd(p, labels) with g == NULL writing loss[1] and z[B] (nullable). labels ==
 * NULL: no loss launch, loss and z are not touched; p is in the workspace.
 *
 * dqrm_model_step (one training step): the forward as above with g[B] written;
 * dqrm_mlp_bwd(top, dy = g) -- loss.backward()'s upstream gradient is 1.0 and 1.0f * g is g bit
 * for bit, so dqrm_loss_bwd is not launched --; dqrm_interact_bwd; dqrm_mlp_bwd(bottom, dx ==
 * NULL); dqrm_emb_bwd_sgd on demb; dqrm_mlp_sgd_multi(bottom, top). dw / db: HOST arrays of device
 * pointers over bottom's layers, then top's. Flags:
 *   DQRM_MODEL_MLP_FRESH  both stacks' integers are current: the forwards run DQRM_MLP_FRESH
 *   DQRM_MODEL_REQUANT    the update refreshes the integers (DQRM_MLP_REQUANT)
 *   DQRM_MODEL_NO_UPDATE  stop after the backward: dw, db and demb are the caller's (the DP hooks),
 *                         no parameter is written; `next` must be NULL
 *   DQRM_MODEL_EMB_READY  the slab already holds this batch's forward (the previous step's `next`):
 *                         dqrm_emb_fwd is skipped
 *   next != NULL          the embedding update is dqrm_emb_bwd_sgd_fwd, which leaves next's forward
 *                         in the slab (one launch when dqrm_bwd_sgd_fwd_is_one_launch); next must
 *                         have batch's num_bags
 * dqrm_model_fwd takes DQRM_MODEL_MLP_FRESH and DQRM_MODEL_EMB_READY.
 *
 * dqrm_model_step_launches: the kernel launches the step will issue (memsets not counted), <0 on
 * arguments the step rejects (workspace and tensor pointers apart). With L = L_bottom + L_top
 * per-channel fresh layers, plain interaction: 3L + 5 (26 for the Kaggle stacks, 4 + 3 layers);
 * - 1 with DQRM_MODEL_EMB_READY; + 1 per quantized per-channel layer and + 2 per per-tensor one
 * when not fresh; + 1 for the quantized interaction's scale; + 1 when DQRM_MODEL_REQUANT meets a
 * per-tensor layer; + 1 when next's forward is a launch of its own; with DQRM_MODEL_NO_UPDATE the
 * two update launches are absent.
 *
 * The whole call is validated before the first launch; a rejected call writes nothing.
 * DQRM_E_INVALID: a null struct or member, what each stage's export rejects, the width rules
 * above (dqrm_batch carries no table count: its arrays are read as the set's T tables', and a
 * caller that knows the count compares it itself), B = batch->num_bags < 1 or > 2^20, unknown flags, null x / labels / loss / g / dw / db, next
 * with another num_bags or with DQRM_MODEL_NO_UPDATE. DQRM_E_WORKSPACE: a null, misaligned or
 * short workspace. No call allocates, synchronises or reads back.
 * ------------------------------------------------------------------------------ */
typedef struct dqrm_model {
    const dqrm_table_set* tables;
    const dqrm_mlp* bottom;
    const dqrm_mlp* top;
    const dqrm_loss* loss;
    dqrm_interact interact;
    int32_t  embedding_bit;   /* dqrm_emb_fwd's bits */
    uint32_t emb_fwd_flags;   /* DQRM_FWD_* of every embedding forward */
    int32_t  ste;             /* dqrm_emb_bwd_sgd's ste (0 with DQRM_FWD_FULL_PRECISION) */
    int32_t  repack_bits;     /* dqrm_emb_bwd_sgd's repack_bits */
} dqrm_model;

typedef struct dqrm_model_layout {  /* byte offsets into the workspace */
    size_t slab, r, p, dr, dx, demb;
    size_t total;                   /* dqrm_model_workspace_bytes */
} dqrm_model_layout;

#define DQRM_MODEL_MLP_FRESH 1u
#define DQRM_MODEL_REQUANT   2u
#define DQRM_MODEL_NO_UPDATE 4u
#define DQRM_MODEL_EMB_READY 8u

/* 0 for arguments it rejects (dqrm_last_error says why) */
size_t dqrm_model_workspace_bytes(const dqrm_model* model, int64_t B, int64_t max_lookups);
int dqrm_model_workspace_layout(const dqrm_model* model, int64_t B, int64_t max_lookups, dqrm_model_layout* out);
int dqrm_model_fwd(const dqrm_model* model, const dqrm_batch* batch, uint32_t flags, const float* x,
                   const float* labels, float* loss, float* z, void* workspace, size_t workspace_bytes,
                   void* stream);
int dqrm_model_step(const dqrm_model* model, const dqrm_batch* batch, const dqrm_batch* next, uint32_t flags,
                    const float* x, const float* labels, float lr, float* loss, float* z, float* g,
                    float* const* dw, float* const* db, void* workspace, size_t workspace_bytes, void* stream);
int dqrm_model_step_launches(const dqrm_model* model, const dqrm_batch* batch, const dqrm_batch* next,
                             uint32_t flags);

/* The quantize_activation model (--quantize_activation, DLRM_Net's quant_input and
 * quant_feature_outputs, dlrm_s_pytorch_tb_dp_one_parallel_comm.py:475-476, :845-876): the calls
 * above with a QuantAct in front of each stack and the stacks' integer-activation forms. The set
 * below is HOST memory and stands beside the model; dqrm_model itself is unchanged. No arithmetic
 * here either: the same shared bodies call the stage exports.
 *
 * Forward: dqrm_emb_fwd; dqrm_act_quant_fwd(quant_input, x -> xq); dqrm_mlp_fwd_qact(bottom, xq,
 * prev = quant_input->scale, out_scale); dqrm_interact_scale / _fwd -> r;
 * dqrm_act_quant_fwd(quant_features, r -> rq); dqrm_mlp_fwd_qact(top, rq, prev =
 * quant_features->scale, out_scale + L_bottom); dqrm_loss_fwd.
 * Backward: dqrm_mlp_bwd_qact(top) with dx; dqrm_act_quant_bwd(quant_features->scale) on it ->
 * dr; dqrm_interact_bwd; dqrm_mlp_bwd_qact(bottom, dx == NULL) -- quant_input's input is data and
 * gets no backward launch --; dqrm_emb_bwd_sgd[_fwd]; dqrm_mlp_sgd_multi. flags, next and
 * DQRM_MODEL_NO_UPDATE mean what they mean above; DQRM_MODEL_MLP_FRESH promises current scales
 * and weight integers, and each stack's forward is then one dqrm_mlp_qact_prepare and its GEMMs.
 * The QuantActs' x_min / x_max / scale are WRITTEN as dqrm_act_quant_fwd writes them
 * (running_stat as each struct says).
 *
 * Act-only mode (the reference's branch at :845-851, QuantActs in front of full-precision MLPs):
 * when every layer of both stacks has quantized[i] == 0 the stacks run dqrm_mlp_fwd / _bwd on
 * xq / rq and out_scale is not read (it may be NULL). A mixture of quantized and full-precision
 * layers is rejected.
 *
 * Workspace: dqrm_model_qact_workspace_bytes; dqrm_model_step's cut comes first, at its offsets
 * (dqrm_model_qact_workspace_layout reports the same members, `total` the longer size), then
 * xq [B][in_bottom], rq [B][R], the two dqrm_act_quant workspaces and the [B][R] gradient in
 * front of quant_features' backward.
 *
 * dqrm_model_qact_step_launches: dqrm_model_step_launches' count with, for integer stacks, the
 * not-fresh weight quantization per layer as there (1 per channel, 2 per tensor) and, fresh, + 2
 * (one prepare per stack); + the two QuantAct forwards (each 1 without running_stat, 2 up to
 * 16384 elements, 3 above) + 1 for quant_features' backward. Fresh per-tensor stacks of L layers
 * in all, a plain interaction and DQRM_MODEL_REQUANT: 3L + a_in + a_feat + 9.
 *
 * DQRM_E_INVALID before any launch: everything the calls above reject; a null set or QuantAct;
 * what dqrm_act_quant_fwd rejects in either struct; for integer stacks what dqrm_mlp_fwd_qact
 * rejects (per_channel on any layer but a stack's last, a null out_scale array or entry). */
typedef struct dqrm_model_qact {
    const dqrm_act_quant* quant_input;     /* in front of the bottom stack */
    const dqrm_act_quant* quant_features;  /* quant_feature_outputs, in front of the top stack */
    float* const* out_scale;               /* HOST [L_bottom + L_top] device pointers: bottom's layers, then top's */
} dqrm_model_qact;

size_t dqrm_model_qact_workspace_bytes(const dqrm_model* model, const dqrm_model_qact* qact, int64_t B,
                                       int64_t max_lookups);
int dqrm_model_qact_workspace_layout(const dqrm_model* model, const dqrm_model_qact* qact, int64_t B,
                                     int64_t max_lookups, dqrm_model_layout* out);
int dqrm_model_fwd_qact(const dqrm_model* model, const dqrm_model_qact* qact, const dqrm_batch* batch,
                        uint32_t flags, const float* x, const float* labels, float* loss, float* z,
                        void* workspace, size_t workspace_bytes, void* stream);
int dqrm_model_step_qact(const dqrm_model* model, const dqrm_model_qact* qact, const dqrm_batch* batch,
                         const dqrm_batch* next, uint32_t flags, const float* x, const float* labels, float lr,
                         float* loss, float* z, float* g, float* const* dw, float* const* db, void* workspace,
                         size_t workspace_bytes, void* stream);
int dqrm_model_qact_step_launches(const dqrm_model* model, const dqrm_model_qact* qact, const dqrm_batch* batch,
                                  const dqrm_batch* next, uint32_t flags);

/* ---------------------------------------------------------------------------------
 * DLRMMetrics: the two numbers of the reference's test loop, test accuracy and ROC AUC
 * (inference(), dlrm_s_pytorch_tb_dp_one_parallel_comm.py:1304-1404), kept on the device,
 * csrc/dqrm_metrics.hip. Per test batch the reference synchronises, copies scores and targets
 * to the host (:1348-1355), counts np.round(S, 0) == T (:1358-1360) and at the end calls
 * sklearn.metrics.roc_auc_score on the concatenated arrays (:1387). Here a batch is one launch
 * that nothing waits for, and the end is a fixed number of launches plus one 40-byte result.
 *
 * The arithmetic, for a stream of (z, t) pairs, both f32:
 *   n_correct  #{ rintf(z) == t }: np.round(S, 0) == T in f32, ties to even (0.5 -> 0, 1.5 -> 2)
 *   key        s = z + 0.0f (-0 ties with +0, as in sklearn); b = bits(s);
 *              key = b >> 31 ? ~b : b | 0x80000000: a uint32 whose unsigned order is the order of
 *              the finite floats
 *   class      t == 1.0f positive, t == 0.0f negative; any other t sets DQRM_METRICS_F_LABEL (the
 *              sample enters neither class); a non-finite z sets DQRM_METRICS_F_NONFINITE. A
 *              flagged sample still counts in the caller's n; a set flag makes the result invalid
 *   twice_u    sum over positives i of 2 * #{negatives j: key_j < key_i} + #{negatives j: key_j ==
 *              key_i}, a uint64: twice the Mann-Whitney U with ties counted one half
 *   roc_auc    twice_u / (2 * n_pos * n_neg), ONE float64 division, done by the caller: the area
 *              sklearn's trapezoid over roc_curve computes
 * Nothing on the device is floating-point arithmetic except rintf, the compares and + 0.0f, and
 * every sum is an integer sum. Where a key lands in `keys` depends on the order in which waves
 * arrive; n_pos, n_neg, n_correct, twice_u and flags are functions of the MULTISET of samples
 * alone: batch order, batch size, grid and arrival order do not enter their bits.
 *
 * State (the struct is HOST memory, its pointers device memory): keys[capacity], positives
 * appended from the front, negatives from the back; counters[4] = n_pos, n_neg, n_correct, flags.
 * dqrm_metrics_reset zeroes the counters (one 32-byte memset, no launch).
 *
 * dqrm_metrics_update (the loop body, :1348-1360): ONE launch for a batch of n samples, z[n] and
 * t[n]. seen_before: the samples of the updates since the reset (the caller's sum of batch
 * sizes). A wave reserves its range with a ballot count and one returning device-scope atomic add
 * per class; n_correct and the flags take one integer atomic per workgroup.
 *
 * dqrm_metrics_finish (:1366, :1387): seen = the samples of all updates since the reset, known to
 * the host, so every grid is sized from it and nothing is read back. The kernels read n_pos and
 * n_neg from the counters, sort the SMALLER class (at most seen / 2 keys; n_pos == n_neg: the
 * positives) in place by an LSD radix sort of four 8-bit passes that ping-pongs through the
 * workspace (per pass: tile histograms of DQRM_METRICS_SORT_TILE keys, a scan, a stable scatter;
 * bare keys without payload, so the sorted bytes are those of any correct sort), then every
 * element of the other class does a lower-bound and an upper-bound search (lb, ub) in it: a
 * positive adds lb + ub when the negatives are sorted, a negative adds 2 * n_pos - lb - ub when
 * the positives are; both sums are twice_u. The last launch writes *out_dev. Surplus workgroups
 * exit. The state stays valid (the order inside a class is not part of it): updates may follow
 * and finish may be called again. Counters that contradict `seen` or `capacity` (a caller that
 * passed wrong counts) set DQRM_METRICS_F_COUNT in the result; nothing is then sorted.
 * dqrm_metrics_finish_launches: its kernel launches (a constant for every valid seen), <0 for
 * seen < 1.
 *
 * workspace: 16-byte aligned, dqrm_metrics_workspace_bytes(seen) bytes (0 for seen outside
 * 1..DQRM_METRICS_MAX_SAMPLES), contents irrelevant; the size grows with seen.
 *
 * Every argument is checked before any launch: a rejected call writes nothing. DQRM_E_INVALID: a
 * null struct or member, capacity outside 1..DQRM_METRICS_MAX_SAMPLES, null z / t / out_dev,
 * n < 1, seen_before < 0, seen_before + n > capacity, seen < 1 or > capacity. DQRM_E_WORKSPACE: a
 * null, misaligned or short workspace. No call allocates, synchronises or reads back.
 * ------------------------------------------------------------------------------ */
#define DQRM_METRICS_MAX_SAMPLES (1ll << 30)
#define DQRM_METRICS_SORT_TILE   4096   /* keys per workgroup of a sort pass */
#define DQRM_METRICS_F_LABEL     1u     /* a target that is neither 0.0f nor 1.0f */
#define DQRM_METRICS_F_NONFINITE 2u     /* a NaN or infinite score */
#define DQRM_METRICS_F_COUNT     4u     /* the device counters contradict seen / capacity */

typedef struct dqrm_metrics {
    int64_t   capacity;    /* samples `keys` holds, 1..DQRM_METRICS_MAX_SAMPLES */
    uint32_t* keys;        /* [capacity] */
    uint64_t* counters;    /* [4] n_pos, n_neg, n_correct, flags */
} dqrm_metrics;

typedef struct dqrm_metrics_result {
    uint64_t n_pos, n_neg, n_correct, twice_u, flags;
} dqrm_metrics_result;

/* test_accu = 0, scores = [], targets = [] (:1317-1321): a 32-byte memset, no launch. */
int dqrm_metrics_reset(const dqrm_metrics* m, void* stream);
/* The loop body after the forward (:1347-1361): no synchronize, no copy; one launch. */
int dqrm_metrics_update(const dqrm_metrics* m, const float* z, const float* t, int64_t n, int64_t seen_before,
                        void* stream);
/* 0 for seen outside 1..DQRM_METRICS_MAX_SAMPLES (dqrm_last_error says why). */
size_t dqrm_metrics_workspace_bytes(int64_t seen);
/* acc_test's numerator (:1366) and np.concatenate + roc_auc_score (:1385-1387) as integers in
 * *out_dev (device memory, 40 bytes); the two divisions are the caller's. */
int dqrm_metrics_finish(const dqrm_metrics* m, int64_t seen, dqrm_metrics_result* out_dev, void* ws,
                        size_t ws_bytes, void* stream);
/* Kernel launches of dqrm_metrics_finish (memsets not counted), <0 for seen it rejects. */
int dqrm_metrics_finish_launches(int64_t seen);

/* ---------------------------------------------------------------------------------
 * Row-wise PTQ formats of the reference's inference path.
 * DLRM_Net.quantize_embedding (dlrm_s_pytorch_single_gpu_documentingp.py:689-704) packs
 * each trained table with torch.ops.quantized.embedding_bag_{4bit,byte}_prepack and
 * apply_emb (:648-663) gathers with embedding_bag_{4bit,byte}_rowwise_offsets (mode sum,
 * optional per-sample weights). Byte-identical to those ops (FBGEMM fused row-wise):
 *   bits 4: row = D/2 bytes (element 2j low nibble, 2j+1 high) | fp16 scale | fp16 bias
 *   bits 8: row = D bytes | f32 scale | f32 bias
 * dim must be 8, 16, 32, 64, 128 or 256. W is 16-byte aligned, packed 4-byte aligned.
 * ------------------------------------------------------------------------------ */
/* Bytes per packed row (0 if bits/dim unsupported). */
size_t dqrm_rowwise_row_bytes(int bits, int dim);

/* packed[num_rows * row_bytes] <- prepack(W[num_rows, dim] f32).
 * Replaces torch.ops.quantized.embedding_bag_4bit_prepack / embedding_bag_byte_prepack. */
int dqrm_rowwise_prepack(int bits, const float* W, int64_t num_rows, int dim, uint8_t* packed,
                         void* stream);

/* out[num_bags, dim] f32 <- sum over bag b of dequant(packed[idx[i]]) (* per_sample_weights[i]),
 * accumulated in bag order as acc = fma(scale*w, q, acc + bias*w) (FBGEMM EmbeddingSpMDM).
 * Bag b covers idx[off[b] .. off[b+1]); with include_last_offset == 0 the last bag ends at
 * num_lookups, otherwise off has num_bags+1 entries. per_sample_weights may be NULL. Out-of-range indices are
 * skipped and flag DQRM_ERRF_INDEX in *err, bad offsets flag DQRM_ERRF_OFFSET (device
 * word, cleared by the caller). Replaces torch.ops.quantized.embedding_bag_4bit_rowwise_offsets /
 * embedding_bag_byte_rowwise_offsets (mode=0 sum). */
int dqrm_rowwise_bag(int bits, const uint8_t* packed, int64_t num_rows, int dim, const int64_t* idx,
                     int64_t num_lookups, const int64_t* off, int64_t num_bags, int include_last_offset,
                     const float* per_sample_weights, float* out, uint32_t* err, void* stream);

/* ---------------------------------------------------------------------------------
 * The quantized model served from row-wise tables, csrc/dqrm_rowwise.hip and dqrm_model.hip.
 * DLRM_Net.quantize_embedding(bits) (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:683-700) prepacks
 * every table and sets emb_l = None; apply_emb (:639-659) then gathers table after table with
 * embedding_bag_{4bit,byte}_rowwise_offsets. Here all T packed tables are ONE slab
 * u8 [total_rows][dqrm_rowwise_row_bytes(bits, dim)] in dqrm_rowwise_prepack's row layout, table t
 * in rows [row_base[t], row_base[t] + num_rows[t]), and all tables' bags are one launch. (The FP32
 * slab of a dqrm_table_set is [R][D] contiguous and prepacking is per row, so one
 * dqrm_rowwise_prepack over its R rows packs every table.)
 *
 * The struct is HOST memory, its pointers device memory. meta: i64 [2][T], row_base then num_rows
 * (the first two rows of dqrm_table_set.meta serve). err: one word of DQRM_ERRF_* flags, cleared by
 * the caller. packed is 4-byte aligned.
 * ------------------------------------------------------------------------------ */
typedef struct dqrm_rowwise_set {
    int32_t  num_tables;      /* T, 1..256 */
    int32_t  dim;             /* D: 8, 16, 32, 64, 128 or 256 */
    int32_t  bits;            /* 4 or 8 */
    int32_t  reserved;
    int64_t  total_rows;      /* R = sum num_rows */
    const uint8_t* packed;    /* [R][row_bytes] */
    const int64_t* meta;      /* [2][T]: row_base, num_rows */
    uint32_t* err;            /* 1 word, device-side error flags */
} dqrm_rowwise_set;

/* apply_emb's loop over the quantized tables (:639-659) as ONE launch: out[t*out_stride_t +
 * b*out_stride_b + d] (dqrm_emb_fwd's addressing) <- table t's bag b, dqrm_rowwise_bag's
 * arithmetic and bits. batch in either form: DQRM_BATCH_POOLING_ONE (bag b is lookup b of
 * idx[t*B, (t+1)*B); off and idx_base are not read and may be NULL) or idx_base / off[T][B] with
 * the last bag ending at L_t. per_sample_weights: NULL or f32 [sum L_t], parallel to idx. An index
 * outside [0, num_rows[t]) flags DQRM_ERRF_INDEX and contributes nothing; a bad offset pair flags
 * DQRM_ERRF_OFFSET and is clamped as in dqrm_rowwise_bag; no address outside the arrays is formed.
 * out 16-byte aligned, strides multiples of 4 floats. num_bags == 0: nothing is launched. */
int dqrm_rowwise_set_fwd(const dqrm_rowwise_set* set, const dqrm_batch* batch, const float* per_sample_weights,
                         float* out, int64_t out_stride_t, int64_t out_stride_b, void* stream);

/* dqrm_model_fwd with the embedding stage replaced by dqrm_rowwise_set_fwd into the [B][T][D] slab:
 * DLRM_Net.forward after quantize_embedding (:683-700; apply_emb :639-659 applies no fake-quant on
 * top of the row-wise gather, so model->embedding_bit / emb_fwd_flags are ignored). model->tables
 * may be NULL and is never read; rset->dim must be model->interact.dim and rset->num_tables + 1
 * model->interact.num_features. flags: DQRM_MODEL_MLP_FRESH only. Everything else as
 * dqrm_model_fwd: no arithmetic here, validated before the first launch, a rejected call writes
 * nothing (DQRM_E_INVALID / DQRM_E_WORKSPACE as there), nothing allocated or synchronised.
 *
 * The workspace is a forward-only cut, dqrm_model_fwd_rowwise_workspace_bytes(model, rset, B)
 * bytes (0 for arguments it rejects), 16-byte aligned: the slab (offset 0), every layer's output,
 * r, the interaction's scale word and the per-tensor layers' row maxima, each on a 256-byte
 * boundary; no dr / dx / demb and no backward scratch. _workspace_layout fills slab, r, p and
 * total; dr, dx and demb are 0.
 *
 * dqrm_model_fwd_rowwise_launches: 1 (the embedding forward) + L (the stacks' layers) + 1 (the
 * interaction) + 1 for the quantized interaction's scale + 1 with labels + dqrm_model_step_launches'
 * additions when not fresh; <0 on arguments the call rejects (workspace and tensors apart). */
int dqrm_model_fwd_rowwise(const dqrm_model* model, const dqrm_rowwise_set* rset, const dqrm_batch* batch,
                           uint32_t flags, const float* x, const float* labels, float* loss, float* z,
                           void* workspace, size_t workspace_bytes, void* stream);
size_t dqrm_model_fwd_rowwise_workspace_bytes(const dqrm_model* model, const dqrm_rowwise_set* rset, int64_t B);
int dqrm_model_fwd_rowwise_workspace_layout(const dqrm_model* model, const dqrm_rowwise_set* rset, int64_t B,
                                            dqrm_model_layout* out);
int dqrm_model_fwd_rowwise_launches(const dqrm_model* model, const dqrm_rowwise_set* rset, const dqrm_batch* batch,
                                    uint32_t flags, int has_labels);

/* ---------------------------------------------------------------------------------
 * The LSQ and PACT embedding quantizers, csrc/dqrm_quantizers.hip: the two baselines the
 * reference's --quant-mode lsq|pact builds its tables from (quant_learned_step_size_quan.py:65-100
 * with quantizer/lsq.py:18-58; quant_pact_dorefa.py:10-28, 57-112), over a dqrm_table_set and a
 * dqrm_batch like dqrm_emb_fwd: out[t*out_stride_t + b*out_stride_b + d], either batch form
 * (DQRM_BATCH_POOLING_ONE honoured), bag sums f32 adds in bag order from 0, an index outside
 * [0, num_rows[t]) flags DQRM_ERRF_INDEX and contributes nothing, a bad offset pair flags
 * DQRM_ERRF_OFFSET and is clamped. Every named step is one IEEE f32 operation (true divisions,
 * rintf = half to even, nothing contracted). bits: 2..8. All calls validate before the first
 * launch (DQRM_E_INVALID; a short workspace DQRM_E_WORKSPACE; a rejected call writes nothing),
 * allocate nothing, synchronise nothing and read nothing back. num_bags == 0: nothing launched.
 *
 * LSQ quantizes the POOLED output with one learned step s_t per table (step[T], device):
 *   lo = -2^(bits-1), hi = 2^(bits-1)-1, n = B*D, g = (float)(1 / sqrt((double)hi * n)) (host)
 *   sg = s*g;  s_eff = (s - sg) + sg          (the reference's grad_scale(); not always s)
 *   x = the bag sum;  q = x / s_eff;  r = rintf(min(max(q, lo), hi));  y = r * s_eff
 * pooled (nullable: inference) receives x as f32 [T][B][D] for the backward. One launch.
 *
 * dqrm_emb_bwd_lsq, given dy (dqrm_emb_bwd_sgd's addressing) and the forward's pooled and step:
 *   m = lo <= q <= hi (both ends inclusive);  gq = m ? dy * s_eff : 0;  dx = gq / s_eff
 *   S1 = sum_e dy_e * r_e;  S2 = sum_e -gq_e * ((x_e / s_eff) / s_eff);  dstep[t] = (S1 + S2) * g
 * dx f32 [T][B][D] (the per-bag row gradient, to be scattered per lookup by dqrm_emb_bwd_sgd /
 * _lookup_grad with ste = 0) and dstep f32 [T] are overwritten. S1 and S2 are reduced in a fixed
 * shape whose bits depend on (B, D) and the data only: elements e = b*D + d; 4096 strided chains
 * per table (chain c takes e = c, c + 4096, ... in ascending order, acc = fmaf(a_e, b_e, acc)
 * from 0), then a pairwise tree over the chain index (c with c^1, then pairs of pairs, ...). No
 * float atomics, no workgroup waits on another; two launches. The workspace needs
 * dqrm_emb_bwd_lsq_workspace_bytes(T, B, D) bytes (0 for arguments it rejects), 16-byte aligned,
 * no initialisation.
 *
 * PACT / DoReFa maps every gathered weight before the bag sum, k = bits, sc = (float)(2^k - 1),
 * mt = tanhf(tmax_t) -- the table-wide max|tanh(W)|, since tanh is odd and monotone -- so the call
 * reads the set's tmax (which must be current, as for a refreshing dqrm_emb_fwd) and the gathered
 * rows, never the whole table:
 *   t = tanhf(w);  u = t / (2*mt);  a = u + 0.5;  j = rintf(sc * a);  v = 2 * (j / sc) - 1
 * An all-zero table gives NaN (the reference's 0/0). Its backward is the identity STE: dy per
 * lookup, dqrm_emb_bwd_sgd(..., ste = 0). One launch.
 *
 * The _launches queries: the kernels the call launches on these arguments (1, 2 and 1; 0 for an
 * empty batch), <0 for a set or batch the call rejects.
 * ------------------------------------------------------------------------------ */
int dqrm_emb_fwd_lsq(const dqrm_table_set* set, const dqrm_batch* batch, const float* step, int bits, float* out,
                     int64_t out_stride_t, int64_t out_stride_b, float* pooled, void* stream);
int dqrm_emb_fwd_lsq_launches(const dqrm_table_set* set, const dqrm_batch* batch);
size_t dqrm_emb_bwd_lsq_workspace_bytes(int num_tables, int64_t num_bags, int dim);
int dqrm_emb_bwd_lsq(const dqrm_table_set* set, const dqrm_batch* batch, const float* dy, int64_t dy_stride_t,
                     int64_t dy_stride_b, const float* pooled, const float* step, int bits, float* dx, float* dstep,
                     void* workspace, size_t workspace_bytes, void* stream);
int dqrm_emb_bwd_lsq_launches(const dqrm_table_set* set, const dqrm_batch* batch);
int dqrm_emb_fwd_pact(const dqrm_table_set* set, const dqrm_batch* batch, int bits, float* out, int64_t out_stride_t,
                      int64_t out_stride_b, void* stream);
int dqrm_emb_fwd_pact_launches(const dqrm_table_set* set, const dqrm_batch* batch);

/* ---------------------------------------------------------------------------------
 * Criteo input path
 * One record = 40 int32: label, 13 dense, 26 categorical (the flat binary file that
 * data_loader_terabyte.numpy_to_binary writes, :243-280). dqrm_criteo_unpack replaces
 * CriteoBinDataset.__getitem__'s _transform_features (data_loader_terabyte.py:68-87,
 * :227-237) and the Kaggle collate (dlrm_data_pytorch.py:328-345) on a device-resident
 * record block records[num_samples][40]:
 *   dense  f32 [B][13]  = log(float(x_int) + 1)
 *   lS_i   i64 [26][B]  = x_cat (% max_ind_range if > 0, Python remainder), transposed
 *   labels f32 [B]      = float(label)
 *   lS_o   i64 [26][B]  = b (nullable: DQRM_BATCH_POOLING_ONE makes it unnecessary)
 * dense's log is the device logf (<= 2 ulp from torch's CPU log; integers bit-exact).
 * ------------------------------------------------------------------------------ */
#define DQRM_CRITEO_RECORD_INTS 40
#define DQRM_CRITEO_DENSE       13
#define DQRM_CRITEO_SPARSE      26

int dqrm_criteo_unpack(const int32_t* records, int64_t num_samples, int32_t max_ind_range, float* dense,
                       int64_t* lS_i, float* labels, int64_t* lS_o, void* stream);

/* ---------------------------------------------------------------------------------
 * Misc
 * ------------------------------------------------------------------------------ */
/* Synthetic on-device init U(-sqrt(1/n_t), +sqrt(1/n_t)) from a counter-based hash
 * (same distribution as quant_modules_not_quantize_grad.py:273-275; not numpy's stream). */
int dqrm_init_uniform(const dqrm_table_set* set, uint64_t seed, void* stream);

/* ---------------------------------------------------------------------------------
 * Replica synchronisation: weight_syncc (sgd_quantized_gradients_parallel_comm.py:963-970,
 * all_reduce(param, SUM) then param *= 1/N, every 200 iterations of the DP driver,
 * dlrm_s_pytorch_tb_dp_one_parallel_comm.py:1801,1924-1936).
 * ------------------------------------------------------------------------------ */
/* *out (device u64, caller-zeroed) += sum_i mix64(word_i ^ i * 0xD1B54A32D192ED03) over num_words 32-bit
 * words of data (16-B aligned): a position-dependent, order-free 64-bit checksum whose
 * all-gather tells whether every rank holds the same bits. */
int dqrm_checksum64(const void* data, int64_t num_words, uint64_t* out, void* stream);

/* In place, the reference's all-reduce + scale of num_replicas IDENTICAL replicas of data:
 * x = fl(fl(...fl(x + x) + x ...) * inv_n), num_replicas - 1 sequential adds -- the order in
 * which a ring all-reduce (Gloo ring_chunked, RCCL ring) accumulates the ranks. Bit-exact
 * with that all-reduce when every rank holds x; the identity for num_replicas 1, 2 and 4
 * with inv_n = 1/num_replicas (barring overflow of num_replicas * x), not for 3 or 8. */
int dqrm_replica_mean(float* data, int64_t n, int num_replicas, float inv_n, void* stream);

/* ---------------------------------------------------------------------------------
 * The N > 1 exchange over RCCL (xGMI), issued from the library: the reference's 52 blocking
 * Gloo collectives per step (2 per table, sgd_quantized_gradients_parallel_comm.py:865,878)
 * become two ncclAllGather calls per step on a communicator libdqrm owns, each stream-ordered
 * between the step's kernels, with no host round trip in between.
 * ------------------------------------------------------------------------------ */
typedef struct dqrm_comm dqrm_comm;

/* RCCL's unique id (128 bytes) for dqrm_comm_init; called by one rank, which hands it to
 * the others (the Python layer broadcasts it over the torch.distributed process group). The
 * RCCL library is the one already loaded in the process (PyTorch's), else librccl.so.1. */
int dqrm_comm_unique_id(void* id128);

/* Collective over the `nranks` processes (one per GPU, each with the same id): creates this
 * rank's communicator on the current HIP device. nranks == 1 is allowed (local copies). */
int dqrm_comm_init(dqrm_comm** comm, int nranks, int rank, const void* id128);

/* A communicator whose all-gather the caller serves: every dqrm_comm_allgather on it (and so
 * both collectives of dqrm_exchange_grad) calls fn(send, recv, bytes, stream, user) on the
 * issuing host thread, with the device pointers and the stream the call was given, in the
 * step's order. fn must leave recv[r * bytes, (r+1) * bytes) = rank r's send in stream order
 * before the stream's next work (e.g. a torch.distributed all_gather_into_tensor on that
 * stream, or a Gloo gather staged through host memory after a stream synchronise) and return
 * 0, else non-zero (the exchange call then fails with DQRM_E_HIP). The exchange's kernels and
 * buffer handling are those of the RCCL communicator: this is how the N > 1 orchestration runs
 * over the reference's own transport (Gloo, s_q_g_p_c.py:865,878) or torch.distributed's. */
typedef int (*dqrm_allgather_fn)(const void* send, void* recv, size_t bytes, void* stream, void* user);
int dqrm_comm_init_external(dqrm_comm** comm, int nranks, int rank, dqrm_allgather_fn fn, void* user);
int dqrm_comm_destroy(dqrm_comm* comm);
int dqrm_comm_size(const dqrm_comm* comm);

/* recv[r * bytes, (r+1) * bytes) <- rank r's send[0, bytes), in rank order, on `stream`
 * (ncclAllGather of bytes uint8). */
int dqrm_comm_allgather(dqrm_comm* comm, const void* send, void* recv, size_t bytes, void* stream);

/* One rank's exchange state, all device buffers caller-owned and reused every step (the
 * Python SparseGradExchange builds it once). */
typedef struct dqrm_exchange {
    const dqrm_table_set* set;
    dqrm_comm* comm;            /* NULL: world size 1, no collective (num_ranks must be 1) */
    int32_t num_ranks;          /* the communicator's size */
    int32_t grad_bits;          /* 2..16 quantized, 32 = the unquantized FP32 path */
    const int64_t* ws_cap_base; /* the coalesced-gradient workspace (dqrm_emb_bwd_coalesce) */
    int64_t ws_cap_total;
    int32_t* ws_rows;
    float* ws_vals;
    int32_t* ws_ucount;
    float* ws_absmax;           /* [T*S] this rank's per-slot max|grad| */
    float* absmax_all;          /* [num_ranks][T*S] gathered maxima (world size 1 without comm: ws_absmax) */
    const int64_t* cap_base;    /* [T+1] payload capacity prefix */
    int64_t cap_total;
    float* s_avg;               /* [T] the averaged gradient scale (emb_scaling_factor) */
    void* payload;              /* this rank's wire payload, dqrm_payload_bytes */
    void* gathered;             /* [num_ranks][payload_bytes] (world size 1 without comm: payload) */
    size_t payload_bytes;
    void* workspace;            /* backward scratch, dqrm_bwd_workspace_bytes(T, max_lookups) */
    size_t workspace_bytes;
    void* apply_ws;             /* the merge apply's positions, dqrm_apply_workspace_bytes(num_ranks,
                                   cap_total); NULL / too small: the flat apply kernel */
    size_t apply_ws_bytes;
} dqrm_exchange;

/* grad_update_parallel_comm's embedding branch for all tables (s_q_g_p_c.py:257-317 via
 * quantize_emb_grad :850-890) in one call: dqrm_emb_bwd_coalesce -> all-gather of the per-slot
 * maxima -> dqrm_grad_quant_pack_strided (rank scales averaged in Gloo's order) -> all-gather
 * of the payloads. Same results as those calls made one by one. */
int dqrm_exchange_grad(const dqrm_exchange* x, const dqrm_batch* batch, const float* dy,
                       int64_t dy_stride_t, int64_t dy_stride_b, int ste, void* stream);

/* weight_update_parallel_comm's embedding branch (s_q_g_p_c.py:601-628): decode the gathered
 * payloads and apply (dqrm_apply_sparse_update_strided with mode / repack_bits). */
int dqrm_exchange_apply(const dqrm_exchange* x, float lr, int mode, int repack_bits, void* stream);

/* dqrm_exchange_apply followed by the NEXT batch's forward, dqrm_emb_fwd(x->set, next, fwd_bits,
 * fwd_flags, out, out_stride_t, out_stride_b): dqrm_apply_sparse_update_fwd on the gathered
 * payloads -- the update of step i and apply_emb of step i+1, adjacent in the DP loop
 * (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:1888-1904, then the next iteration's forward). */
int dqrm_exchange_apply_fwd(const dqrm_exchange* x, float lr, int mode, int repack_bits, const dqrm_batch* next,
                            int fwd_bits, uint32_t fwd_flags, float* out, int64_t out_stride_t, int64_t out_stride_b,
                            void* stream);

/* dqrm_emb_bwd_lookup_grad with duplicate rows pre-summed: same rows[], but vals[j] is the
 * sum, in lookup order, of the STE'd dy rows of every lookup of row idx[j] when j is the
 * row's FIRST lookup, and +0.0 for its later lookups. Handed to torch.optim.SGD
 * (dlrm_s_pytorch_single_gpu.py:1943-1950) the scatter-add then adds one value per row
 * (a zero entry adds -lr * 0 = -0.0, the identity), so W is bit-identical run to run;
 * the COO sums to the same per-row gradient. Tables of more than DQRM_PRESUM_MAX_LOOKUPS
 * lookups: DQRM_E_CAPACITY (nothing written). */
#define DQRM_PRESUM_MAX_LOOKUPS 2048
int dqrm_emb_bwd_lookup_grad_presum(const dqrm_table_set* set, const dqrm_batch* batch, const float* dy,
                                    int64_t dy_stride_t, int64_t dy_stride_b, int ste, int64_t* rows,
                                    float* vals, void* stream);

/* Synchronises `stream`, returns the accumulated DQRM_ERRF_* flags in *flags and
 * clears them (if clear != 0). */
int dqrm_read_errors(const dqrm_table_set* set, uint32_t* flags, int clear, void* stream);

const char* dqrm_last_error(void);
int dqrm_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DQRM_H_ */
