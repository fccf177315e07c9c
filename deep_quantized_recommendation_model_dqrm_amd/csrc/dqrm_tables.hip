// dqrm_tables.hip — the table set's state outside the training step: the synthetic init (K0), the
// |W| absolute-max hierarchy built from scratch (K1), and the periodic scale refresh with its
// conditional INT4 repack (K2). Streaming passes over the slab, HBM-bound, no LDS beyond a
// workgroup reduction. (Inside the step the hierarchy is kept by the apply kernels and
// finalize_table, dqrm_device.h.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dqrm_device.h"
#include "dqrm_internal.h"

namespace {

using dqrm_internal::check_set;
using dqrm_internal::grid_for;
using dqrm_internal::set_error;

// ------------------------------------------------------------------------------------
// K0: synthetic init, U(-sqrt(1/n), sqrt(1/n)) per table (q_m_n_q_g.py:273-275 distribution)
// ------------------------------------------------------------------------------------
DQRM_INLINE uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ void k_init_uniform(float* __restrict__ W, const int64_t* __restrict__ meta, int T,
                               int D, int64_t total_rows, uint64_t seed) {
    Meta m = make_meta(meta, T);
    const int64_t n4 = total_rows * (D / 4);
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4;
         q += (int64_t)gridDim.x * blockDim.x) {
        int64_t row = q / (D / 4);
        int t = find_table(m.row_base, T, row);
        float bound = sqrtf(1.0f / (float)m.num_rows[t]);
        uint64_t h0 = splitmix64(seed ^ ((uint64_t)q * 2ull));
        uint64_t h1 = splitmix64(seed ^ ((uint64_t)q * 2ull + 1ull));
        float4 v;
        v.x = ((float)(uint32_t)(h0 >> 40) * (1.0f / 16777216.0f)) * 2.0f - 1.0f;
        v.y = ((float)(uint32_t)((h0 >> 16) & 0xFFFFFF) * (1.0f / 16777216.0f)) * 2.0f - 1.0f;
        v.z = ((float)(uint32_t)(h1 >> 40) * (1.0f / 16777216.0f)) * 2.0f - 1.0f;
        v.w = ((float)(uint32_t)((h1 >> 16) & 0xFFFFFF) * (1.0f / 16777216.0f)) * 2.0f - 1.0f;
        v.x *= bound; v.y *= bound; v.z *= bound; v.w *= bound;
        reinterpret_cast<float4*>(W)[q] = v;
    }
}

// ------------------------------------------------------------------------------------
// K1: absolute-max hierarchy  rowmax -> blkmax -> sblkmax -> tmax
// (exact replacement of the full-table min/max, quant_utils.py:177-178)
// ------------------------------------------------------------------------------------
template <int LPR>  // lanes per row = D/4
__global__ void k_rowmax_all(const float* __restrict__ W, float* __restrict__ rowmax,
                             int64_t total_rows) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ngrp = (int64_t)gridDim.x * blockDim.x / LPR;
    const int lane = threadIdx.x % LPR;
    for (int64_t row = gid / LPR; row < total_rows; row += ngrp) {
        float4 v = reinterpret_cast<const float4*>(W + row * (LPR * 4))[lane];
        float m = group_max<LPR>(abs_max4(v));
        if (lane == 0) rowmax[row] = m;
    }
}

// one wave per output: out[ob_t + j] = max(in[ib_t + j*256 .. min(+256, nin_t)])
// level 1: in = rowmax (ib = row_base, nin = num_rows), out = blkmax (ob = blk_base)
// level 2: in = blkmax (ib = blk_base, nin = nblk),     out = sblkmax (ob = sblk_base)
__global__ void k_level_max(const float* __restrict__ in, float* __restrict__ out,
                            const int64_t* __restrict__ meta, int T, int level,
                            int64_t total_out) {
    Meta m = make_meta(meta, T);
    const int lane = threadIdx.x % WAVE;
    const int64_t wid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int64_t nw = (int64_t)gridDim.x * blockDim.x / WAVE;
    const int64_t* ob = level == 1 ? m.blk_base : m.sblk_base;
    for (int64_t o = wid; o < total_out; o += nw) {
        int t = find_table(ob, T, o);
        int64_t j = o - ob[t];
        int64_t ib = level == 1 ? m.row_base[t] : m.blk_base[t];
        int64_t nin = level == 1 ? m.num_rows[t] : ceil_div(m.num_rows[t], BLK);
        int64_t s0 = j * 256, s1 = s0 + 256 < nin ? s0 + 256 : nin;
        float v = 0.0f;
        for (int64_t k = s0 + lane; k < s1; k += WAVE) v = fmaxf(v, in[ib + k]);
        v = wave_max(v);
        if (lane == 0) out[o] = v;
    }
}

// one workgroup per table: tmax[t] = max(sblkmax of t)
__global__ void k_table_max(const float* __restrict__ sblkmax, float* __restrict__ tmax,
                            const int64_t* __restrict__ meta, int T) {
    Meta m = make_meta(meta, T);
    __shared__ float red[16];
    const int t = blockIdx.x;
    const int64_t ns = ceil_div(ceil_div(m.num_rows[t], BLK), SBLK_BLOCKS);
    float v = 0.0f;
    for (int64_t k = threadIdx.x; k < ns; k += blockDim.x) v = fmaxf(v, sblkmax[m.sblk_base[t] + k]);
    v = wave_max(v);
    if ((threadIdx.x % WAVE) == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = 0.0f;
        for (int w = 0; w < (int)(blockDim.x / WAVE); ++w) r = fmaxf(r, red[w]);
        tmax[t] = r;
    }
}

// ------------------------------------------------------------------------------------
// K2: periodic scale refresh + conditional INT4 repack
// ------------------------------------------------------------------------------------
__global__ void k_refresh_scale(const float* __restrict__ tmax, float* __restrict__ scale,
                                float* __restrict__ pscale, uint32_t* __restrict__ tflags,
                                int T, int bits, int has_packed) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    float s = sym_scale(tmax[t], bits);
    scale[t] = s;
    uint32_t need = 0;
    if (has_packed) {
        float ps = pscale[t];
        need = !(ps == s);  // NaN pscale (never packed) -> repack
        pscale[t] = s;
    }
    tflags[t] = need;
}

template <int LPR>
__global__ void k_repack_flagged(const float* __restrict__ W, uint8_t* __restrict__ packed,
                                 const float* __restrict__ scale,
                                 const uint32_t* __restrict__ tflags,
                                 const int64_t* __restrict__ meta, int T, int64_t total_rows) {
    Meta m = make_meta(meta, T);
    const int lane = threadIdx.x % LPR;
    const int64_t ngrp = (int64_t)gridDim.x * blockDim.x / LPR;
    const int64_t g0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LPR;
    for (int t = 0; t < T; ++t) {
        if (!tflags[t]) continue;  // scale unchanged since the last pack: rows still exact
        const float r = 1.0f / scale[t];
        const int64_t r0 = m.row_base[t], r1 = r0 + m.num_rows[t];
        for (int64_t row = r0 + g0; row < r1; row += ngrp) {
            float4 w = reinterpret_cast<const float4*>(W + row * (LPR * 4))[lane];
            pack_row_int4<LPR>(w, packed, row, lane, r);
        }
    }
    (void)total_rows;
}

}  // namespace

extern "C" {

int dqrm_init_uniform(const dqrm_table_set* set, uint64_t seed, void* stream) {
    int rc = check_set(set);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n4 = set->total_rows * (set->dim / 4);
    hipLaunchKernelGGL(k_init_uniform, dim3(grid_for(n4, 256, 8192)), dim3(256), 0, st, set->W,
                       set->meta, set->num_tables, set->dim, set->total_rows, seed);
    LAUNCH_CHECK();
    return DQRM_OK;
}

int dqrm_refresh_absmax(const dqrm_table_set* set, void* stream) {
    int rc = check_set(set);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int D = set->dim;
    DISPATCH_LPR(D, {
        hipLaunchKernelGGL(k_rowmax_all<LPR>, dim3(grid_for(set->total_rows * LPR, 256, 8192)), dim3(256), 0,
                           st, set->W, set->rowmax, set->total_rows);
    });
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_level_max, dim3(grid_for(set->total_blocks * WAVE, 256, 8192)), dim3(256), 0, st,
                       set->rowmax, set->blkmax, set->meta, set->num_tables, 1, set->total_blocks);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_level_max, dim3(grid_for(set->total_sblocks * WAVE, 256, 8192)), dim3(256), 0, st,
                       set->blkmax, set->sblkmax, set->meta, set->num_tables, 2, set->total_sblocks);
    LAUNCH_CHECK();
    DQRM_HIP_TRY(hipMemsetAsync(set->sdirty, 0, (size_t)set->total_sblocks, st));
    DQRM_HIP_TRY(hipMemsetAsync(set->bdirty, 0, (size_t)set->total_blocks, st));
    DQRM_HIP_TRY(hipMemsetAsync(set->sync, 0, (size_t)set->num_tables * DQRM_SYNC_STRIDE * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_table_max, dim3(set->num_tables), dim3(256), 0, st, set->sblkmax, set->tmax,
                       set->meta, set->num_tables);
    LAUNCH_CHECK();
    return DQRM_OK;
}

int dqrm_refresh_scale_and_pack(const dqrm_table_set* set, int bits, void* stream) {
    int rc = check_set(set);
    if (rc) return rc;
    if (bits < 2 || bits > 16) return set_error(DQRM_E_INVALID, "%s: bits %d unsupported", "refresh", bits);
    if (set->packed && bits != 4)
        return set_error(DQRM_E_INVALID, "%s: packed rows need bits == 4 (got %d)", "refresh", bits);
    hipStream_t st = (hipStream_t)stream;
    const int T = set->num_tables;
    hipLaunchKernelGGL(k_refresh_scale, dim3((T + 255) / 256), dim3(256), 0, st, set->tmax, set->scale,
                       set->pscale, set->tflags, T, bits, set->packed != nullptr);
    LAUNCH_CHECK();
    if (set->packed) {
        const int D = set->dim;
        DISPATCH_LPR(D, {
            hipLaunchKernelGGL(k_repack_flagged<LPR>, dim3(grid_for(set->total_rows * LPR, 256, 8192)),
                               dim3(256), 0, st, set->W, set->packed, set->scale, set->tflags, set->meta,
                               T, set->total_rows);
        });
        LAUNCH_CHECK();
    }
    return DQRM_OK;
}

}  // extern "C"
