// dqrm_quantizers.hip — the two embedding-quantization baselines the paper compares DQRM's
// per-table INT4 scheme against, as multi-table EmbeddingBag kernels over a dqrm_table_set:
//
//   LSQ  (quant_learned_step_size_quan.py:65-100, quantizer/lsq.py:18-58): the POOLED output of
//        every table is quantized with one learned step per table; the backward masks the
//        clamp and reduces the step's gradient in a fixed shape (no float atomics).
//   PACT / DoReFa (quant_pact_dorefa.py:10-28, 57-112): every gathered ROW is mapped through
//        tanh onto a 2^k-level grid scaled by the table-wide max|tanh(W)| = tanh(max|W|), which
//        is tanhf of the set's tmax: only the gathered rows are read, never the table.
//
// The gather is k_emb_fwd's (dqrm_kernels.hip): LPR = D/4 lanes x float4 per bag, UNR bags in
// flight per lane group, every load of a phase issued before the first use, bag sums f32 adds
// in bag order from 0. Every arithmetic step below is one separately rounded f32 operation
// (-ffp-contract=off); the only fused multiply-adds are the explicit fmaf chains of the LSQ
// step gradient.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dqrm_device.h"
#include "dqrm_internal.h"

namespace {

using dqrm_internal::check_batch;
using dqrm_internal::check_dy;
using dqrm_internal::check_set;
using dqrm_internal::set_error;

constexpr int Q_TPB = 256;
constexpr int Q_UNR = 4;          // bags in flight per lane group
constexpr int Q_GRID = 8192;      // workgroups in all, as k_emb_fwd; grid-stride beyond

// The LSQ step gradient's reduction shape, per table, elements e = b*D + d:
// LSQ_CHAINS strided fmaf chains (chain c takes e = c, c + LSQ_CHAINS, ... in that order, from
// 0), then a pairwise tree over the chain index (level by level, neighbours c and c ^ 1 first).
// A thread owns 4 adjacent chains (one float4), a workgroup 1024, LSQ_WGS workgroups the table.
constexpr int LSQ_CHAINS = 4096;
constexpr int LSQ_WGS = LSQ_CHAINS / (4 * Q_TPB);  // 4 workgroups per table
constexpr int LSQ_F4 = LSQ_CHAINS / 4;             // float4s per sweep of the chains
static_assert(LSQ_WGS == 4, "k_lsq_dstep's tree is written for 4 partials per table");

struct QFwdArgs {
    const float* W;
    const float* tmax;
    const float* step;     // LSQ: [T]
    const int64_t* meta;
    uint32_t* err;
    const int64_t* idx;
    const int64_t* off;
    const int64_t* idx_base;
    float* out;
    float* pooled;         // LSQ: [T][B][D] (nullable)
    int64_t B;
    int64_t ost_t, ost_b;
    int T;
    int pool1;
    float lo, hi;          // LSQ: the clamp's ends
    float g;               // LSQ: the step's gradient scale
    float sc;              // PACT: 2^k - 1
    uint32_t wt;           // wt_stores() bits (WT_Y: out is stored write-through)
};

// s_eff of the reference's grad_scale(): (s - s*g) + s*g, which is not always s
DQRM_INLINE float lsq_s_eff(float s, float g) {
    const float sg = s * g;
    return (s - sg) + sg;
}

DQRM_INLINE float lsq_clamp(float q, float lo, float hi) {  // torch.clamp: NaN stays NaN
    return q < lo ? lo : (q > hi ? hi : q);
}

DQRM_INLINE float lsq_quant(float x, float s_eff, float lo, float hi) {
    const float q = x / s_eff;
    return rintf(lsq_clamp(q, lo, hi)) * s_eff;
}

// DoReFa's value of one weight: 2 * (round(sc * (tanh(w) / (2 mt) + 0.5)) / sc) - 1
DQRM_INLINE float pact_value(float w, float mt2, float sc) {
    const float t = tanhf(w);
    const float u = t / mt2;
    const float a = u + 0.5f;
    const float j = rintf(sc * a);
    return 2.0f * (j / sc) - 1.0f;
}

enum { MODE_LSQ = 0, MODE_PACT = 1 };

// One row's contribution to its bag: the row itself (LSQ) or its DoReFa values (PACT)
template <int MODE>
DQRM_INLINE float4 row_value(float4 w, float mt2, float sc) {
    if constexpr (MODE == MODE_PACT) {
        w.x = pact_value(w.x, mt2, sc); w.y = pact_value(w.y, mt2, sc);
        w.z = pact_value(w.z, mt2, sc); w.w = pact_value(w.w, mt2, sc);
    }
    return w;
}

template <int LPR, int MODE>
__global__ void __launch_bounds__(Q_TPB) k_emb_fwd_quantizer(QFwdArgs a) {
    // grid = (bag chunks, tables): every per-table value is wave-uniform
    const int t = blockIdx.y;
    const int64_t bx = blockIdx.x, gx = gridDim.x;
    constexpr int UNR = Q_UNR;
    constexpr int G = Q_TPB / LPR;  // bags per workgroup pass
    constexpr int D = LPR * 4;
    const int lane = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    float s_eff = 1.0f, mt2 = 1.0f;
    if constexpr (MODE == MODE_LSQ) s_eff = lsq_s_eff(a.step[t], a.g);
    else mt2 = 2.0f * tanhf(a.tmax[t]);  // tanh is odd and monotone: max|tanh(W)| = tanh(max|W|)
    const int64_t rowbase = a.meta[t], nrows = a.meta[a.T + t];
    const int64_t ibase = a.pool1 ? (int64_t)t * a.B : a.idx_base[t];
    const int64_t L = a.pool1 ? a.B : a.idx_base[t + 1] - ibase;
    const int64_t B = a.B;
    const int64_t* __restrict__ off = a.off + (int64_t)t * B;
    const int64_t* __restrict__ idx = a.idx + ibase;
    float* __restrict__ out = a.out + (int64_t)t * a.ost_t;
    float* __restrict__ pooled = a.pooled ? a.pooled + (int64_t)t * B * D : nullptr;
    const bool wty = (a.wt & WT_Y) != 0;
    const bool p1 = a.pool1 && L == B;
    // As in emb_fwd_table: the loads of a phase are issued unconditionally on clamped addresses
    // and the values of invalid bags / lookups dropped afterwards, so the UNR bags' loads are in
    // flight together.
    for (int64_t b0 = bx * (G * UNR); b0 < B; b0 += gx * (G * UNR)) {
        int64_t beg[UNR], len[UNR], row[UNR], s0v[UNR], s1v[UNR], rv[UNR];
#pragma unroll
        for (int k = 0; k < UNR; ++k) {  // phase 1: offsets
            const int64_t b = b0 + k * G + grp;
            const int64_t bb = b < B ? b : 0;
            if (p1) {
                s0v[k] = bb;
                s1v[k] = bb + 1;
            } else {
                s0v[k] = off[bb];
                s1v[k] = off[bb + 1 < B ? bb + 1 : bb];
            }
        }
#pragma unroll
        for (int k = 0; k < UNR; ++k) {
            const int64_t b = b0 + k * G + grp;
            const bool valid = b < B;
            int64_t s0 = s0v[k];
            int64_t s1 = (p1 || b + 1 < B) ? s1v[k] : L;
            if (s0 < 0 || s1 > L || s1 < s0) {
                if (valid && lane == 0) flag_error(a.err, DQRM_ERRF_OFFSET);
                s0 = s0 < 0 ? 0 : (s0 > L ? L : s0);
                s1 = s1 < s0 ? s0 : (s1 > L ? L : s1);
            }
            beg[k] = s0;
            len[k] = valid ? s1 - s0 : -1;  // -1: no such bag
        }
#pragma unroll
        for (int k = 0; k < UNR; ++k) rv[k] = L > 0 ? idx[beg[k] < L ? beg[k] : L - 1] : -1;  // phase 2: first index
#pragma unroll
        for (int k = 0; k < UNR; ++k) {
            row[k] = -1;
            if (len[k] >= 1) {
                if (rv[k] < 0 || rv[k] >= nrows) {
                    if (lane == 0) flag_error(a.err, DQRM_ERRF_INDEX);
                } else {
                    row[k] = rv[k];
                }
            }
        }
        float4 acc[UNR];  // phase 3: the bags' first rows (row 0 of the table for the others, dropped)
#pragma unroll
        for (int k = 0; k < UNR; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (nrows > 0) {
#pragma unroll
            for (int k = 0; k < UNR; ++k)
                acc[k] = reinterpret_cast<const float4*>(a.W + (rowbase + (row[k] >= 0 ? row[k] : 0)) * D)[lane];
        }
        // phase 4: bag sums from 0 in bag order, the epilogue, then the stores together (st4_out)
        float4 xs[UNR];
#pragma unroll
        for (int k = 0; k < UNR; ++k) {
            if (len[k] < 0) continue;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row[k] >= 0) {
                const float4 w = row_value<MODE>(acc[k], mt2, a.sc);
                v.x = v.x + w.x; v.y = v.y + w.y; v.z = v.z + w.z; v.w = v.w + w.w;
            }
            for (int64_t i = 1; i < len[k]; ++i) {
                const int64_t rr = idx[beg[k] + i];
                if (rr < 0 || rr >= nrows) {
                    if (lane == 0) flag_error(a.err, DQRM_ERRF_INDEX);
                    continue;
                }
                const float4 w = row_value<MODE>(reinterpret_cast<const float4*>(a.W + (rowbase + rr) * D)[lane],
                                                 mt2, a.sc);
                v.x = v.x + w.x; v.y = v.y + w.y; v.z = v.z + w.z; v.w = v.w + w.w;
            }
            xs[k] = v;
            if constexpr (MODE == MODE_LSQ) {
                v.x = lsq_quant(v.x, s_eff, a.lo, a.hi); v.y = lsq_quant(v.y, s_eff, a.lo, a.hi);
                v.z = lsq_quant(v.z, s_eff, a.lo, a.hi); v.w = lsq_quant(v.w, s_eff, a.lo, a.hi);
            }
            acc[k] = v;
        }
        if constexpr (MODE == MODE_LSQ) {
            if (pooled) {
#pragma unroll
                for (int k = 0; k < UNR; ++k)
                    if (len[k] >= 0) reinterpret_cast<float4*>(pooled + (b0 + k * G + grp) * D)[lane] = xs[k];
            }
        }
#pragma unroll
        for (int k = 0; k < UNR; ++k)
            if (len[k] >= 0) st4_out(reinterpret_cast<float4*>(out + (b0 + k * G + grp) * a.ost_b) + lane, acc[k], wty);
    }
}

// ------------------------------------------------------------------------------------
// LSQ backward: dx, and the step gradient's per-workgroup partial sums
// ------------------------------------------------------------------------------------
struct LsqBwdArgs {
    const float* dy;
    int64_t dst_t, dst_b;
    const float* pooled;   // [T][B][D]
    const float* step;     // [T]
    float* dx;             // [T][B][D]
    float* part;           // [T][LSQ_WGS][2]: S1, S2 of the workgroup's 1024 chains
    int64_t n4;            // B * D / 4 float4s per table
    int lpr_shift;         // log2(D / 4)
    float lo, hi, g;
};

struct LsqElem {
    float dx, r, gq, qs;   // dx; rint(clamp(q)); the masked gradient; (x / s_eff) / s_eff
};

DQRM_INLINE LsqElem lsq_elem(float x, float dy, float s_eff, float lo, float hi) {
    LsqElem e;
    const float q = x / s_eff;
    const bool m = q >= lo && q <= hi;  // both ends inclusive; NaN is outside
    e.r = rintf(lsq_clamp(q, lo, hi));
    e.gq = m ? dy * s_eff : 0.0f;
    e.dx = e.gq / s_eff;
    e.qs = q / s_eff;
    return e;
}

__global__ void __launch_bounds__(Q_TPB) k_lsq_bwd(LsqBwdArgs a) {
    __shared__ float s_red[2][Q_TPB / WAVE];
    const int t = blockIdx.y, w = blockIdx.x;
    const float s_eff = lsq_s_eff(a.step[t], a.g);
    const float* __restrict__ dy = a.dy + (int64_t)t * a.dst_t;
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(a.pooled) + (int64_t)t * a.n4;
    float4* __restrict__ dx4 = reinterpret_cast<float4*>(a.dx) + (int64_t)t * a.n4;
    const int64_t lpr_mask = (1ll << a.lpr_shift) - 1;
    float c1[4] = {0.f, 0.f, 0.f, 0.f}, c2[4] = {0.f, 0.f, 0.f, 0.f};  // this thread's 4 chains of S1, S2
    constexpr int U = 4;  // sweeps in flight
    for (int64_t f0 = (int64_t)w * Q_TPB + threadIdx.x; f0 < a.n4; f0 += (int64_t)U * LSQ_F4) {
        float4 xv[U], gv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t f = f0 + (int64_t)u * LSQ_F4;
            const int64_t fc = f < a.n4 ? f : f0;  // clamped: loaded, dropped
            xv[u] = x4[fc];
            gv[u] = reinterpret_cast<const float4*>(dy + (fc >> a.lpr_shift) * a.dst_b)[fc & lpr_mask];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {  // in sweep order: a chain's elements in ascending e
            const int64_t f = f0 + (int64_t)u * LSQ_F4;
            if (f >= a.n4) break;
            const float xe[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w};
            const float ge[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w};
            float de[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const LsqElem e = lsq_elem(xe[j], ge[j], s_eff, a.lo, a.hi);
                de[j] = e.dx;
                c1[j] = fmaf(ge[j], e.r, c1[j]);
                c2[j] = fmaf(-e.gq, e.qs, c2[j]);
            }
            dx4[f] = make_float4(de[0], de[1], de[2], de[3]);
        }
    }
    // the tree over the chain index: the thread's 4 chains, the wave's 64 threads (xor 1, 2, ..,
    // 32: both partners compute the same a + b), the workgroup's 4 waves
    float v1 = (c1[0] + c1[1]) + (c1[2] + c1[3]);
    float v2 = (c2[0] + c2[1]) + (c2[2] + c2[3]);
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        v1 = v1 + __shfl_xor(v1, m, WAVE);
        v2 = v2 + __shfl_xor(v2, m, WAVE);
    }
    if (threadIdx.x % WAVE == 0) {
        s_red[0][threadIdx.x / WAVE] = v1;
        s_red[1][threadIdx.x / WAVE] = v2;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const float* r = s_red[threadIdx.x];
        a.part[((int64_t)t * LSQ_WGS + w) * 2 + threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
    }
}

// the tree's last two levels over a table's LSQ_WGS partials, then ds = (S1 + S2) * g
__global__ void __launch_bounds__(Q_TPB) k_lsq_dstep(const float* part, float* dstep, int T, float g) {
    const int t = blockIdx.x * Q_TPB + threadIdx.x;
    if (t >= T) return;
    const float* p = part + (int64_t)t * LSQ_WGS * 2;
    const float s1 = (p[0] + p[2]) + (p[4] + p[6]);
    const float s2 = (p[1] + p[3]) + (p[5] + p[7]);
    dstep[t] = (s1 + s2) * g;
}

// ---- host side
int check_bits(int bits, const char* who) {
    if (bits < 2 || bits > 8) return set_error(DQRM_E_INVALID, "%s: bits must be 2..8 (got %d)", who, bits);
    return DQRM_OK;
}

int check_out(const float* out, int64_t out_stride_t, int64_t out_stride_b, const char* who) {
    if (!out || (((uintptr_t)out) & 15) || (out_stride_t & 3) || (out_stride_b & 3))
        return set_error(DQRM_E_INVALID, "%s: out must be non-null, 16-B aligned with strides %% 4 == 0", who);
    return DQRM_OK;
}

// g = 1 / sqrt(hi * n), n = B * D: in double, rounded once (the reference's Python float)
float lsq_grad_scale(int bits, int64_t B, int D) {
    const double hi = (double)((1 << (bits - 1)) - 1);
    return (float)(1.0 / sqrt(hi * (double)(B * (int64_t)D)));
}

QFwdArgs fwd_args(const dqrm_table_set* set, const dqrm_batch* batch, float* out, int64_t ost_t, int64_t ost_b) {
    QFwdArgs a{};
    a.W = set->W; a.tmax = set->tmax; a.meta = set->meta; a.err = set->err;
    a.idx = batch->idx; a.off = batch->off; a.idx_base = batch->idx_base;
    a.out = out; a.B = batch->num_bags; a.ost_t = ost_t; a.ost_b = ost_b; a.T = set->num_tables;
    a.pool1 = (batch->flags & DQRM_BATCH_POOLING_ONE) != 0;
    a.wt = dqrm_internal::wt_stores(set->dim);
    return a;
}

template <int MODE>
int launch_fwd(const QFwdArgs& a, int D, hipStream_t st) {
    DISPATCH_LPR(D, {
        constexpr int BAGS_PER_WG = (Q_TPB / LPR) * Q_UNR;
        int64_t bx = (a.B + BAGS_PER_WG - 1) / BAGS_PER_WG;
        const int64_t cap = (Q_GRID + a.T - 1) / a.T;
        if (bx > cap) bx = cap;
        hipLaunchKernelGGL((k_emb_fwd_quantizer<LPR, MODE>), dim3((unsigned)bx, (unsigned)a.T), dim3(Q_TPB), 0, st, a);
    });
    LAUNCH_CHECK();
    return DQRM_OK;
}

int check_set_batch(const dqrm_table_set* set, const dqrm_batch* batch, const char* who) {
    int rc = check_set(set);
    if (rc) return rc;
    return check_batch(batch, who);
}

}  // namespace

extern "C" {

int dqrm_emb_fwd_lsq(const dqrm_table_set* set, const dqrm_batch* batch, const float* step, int bits, float* out,
                     int64_t out_stride_t, int64_t out_stride_b, float* pooled, void* stream) {
    const char* who = "dqrm_emb_fwd_lsq";
    int rc = check_set_batch(set, batch, who);
    if (rc) return rc;
    if ((rc = check_bits(bits, who))) return rc;
    if (!step) return set_error(DQRM_E_INVALID, "%s: null step", who);
    if ((rc = check_out(out, out_stride_t, out_stride_b, who))) return rc;
    if (((uintptr_t)pooled) & 15) return set_error(DQRM_E_INVALID, "%s: pooled must be 16-B aligned", who);
    if (batch->num_bags <= 0) return DQRM_OK;
    QFwdArgs a = fwd_args(set, batch, out, out_stride_t, out_stride_b);
    a.step = step;
    a.pooled = pooled;
    a.lo = -(float)(1 << (bits - 1));
    a.hi = (float)((1 << (bits - 1)) - 1);
    a.g = lsq_grad_scale(bits, batch->num_bags, set->dim);
    return launch_fwd<MODE_LSQ>(a, set->dim, (hipStream_t)stream);
}

int dqrm_emb_fwd_lsq_launches(const dqrm_table_set* set, const dqrm_batch* batch) {
    const int rc = check_set_batch(set, batch, "dqrm_emb_fwd_lsq_launches");
    if (rc) return rc;
    return batch->num_bags > 0 ? 1 : 0;
}

size_t dqrm_emb_bwd_lsq_workspace_bytes(int num_tables, int64_t num_bags, int dim) {
    if (num_tables <= 0 || num_tables > dqrm_internal::kMaxTables || num_bags < 0 || dim < 4 || dim > 256 || (dim & 3) ||
        ((dim / 4) & (dim / 4 - 1)))
        return 0;
    return (size_t)num_tables * LSQ_WGS * 2 * sizeof(float);
}

int dqrm_emb_bwd_lsq(const dqrm_table_set* set, const dqrm_batch* batch, const float* dy, int64_t dy_stride_t,
                     int64_t dy_stride_b, const float* pooled, const float* step, int bits, float* dx, float* dstep,
                     void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "dqrm_emb_bwd_lsq";
    int rc = check_set_batch(set, batch, who);
    if (rc) return rc;
    if ((rc = check_bits(bits, who))) return rc;
    if ((rc = check_dy(dy, dy_stride_t, dy_stride_b, who))) return rc;
    if (!step || !dstep) return set_error(DQRM_E_INVALID, "%s: null step / dstep", who);
    if (!pooled || !dx || (((uintptr_t)pooled) & 15) || (((uintptr_t)dx) & 15))
        return set_error(DQRM_E_INVALID, "%s: pooled / dx must be non-null and 16-B aligned", who);
    if (!workspace || (((uintptr_t)workspace) & 15))
        return set_error(DQRM_E_INVALID, "%s: null / unaligned workspace", who);
    if (workspace_bytes < dqrm_emb_bwd_lsq_workspace_bytes(set->num_tables, batch->num_bags, set->dim))
        return set_error(DQRM_E_WORKSPACE, "%s: workspace too small (%zu bytes)", who, workspace_bytes);
    if (batch->num_bags <= 0) return DQRM_OK;
    const int D = set->dim, T = set->num_tables;
    LsqBwdArgs a{};
    a.dy = dy; a.dst_t = dy_stride_t; a.dst_b = dy_stride_b; a.pooled = pooled; a.step = step; a.dx = dx;
    a.part = (float*)workspace;
    a.n4 = batch->num_bags * (int64_t)(D / 4);
    a.lpr_shift = __builtin_ctz((unsigned)(D / 4));
    a.lo = -(float)(1 << (bits - 1));
    a.hi = (float)((1 << (bits - 1)) - 1);
    a.g = lsq_grad_scale(bits, batch->num_bags, D);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_lsq_bwd, dim3(LSQ_WGS, (unsigned)T), dim3(Q_TPB), 0, st, a);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_lsq_dstep, dim3((unsigned)((T + Q_TPB - 1) / Q_TPB)), dim3(Q_TPB), 0, st,
                       (const float*)a.part, dstep, T, a.g);
    LAUNCH_CHECK();
    return DQRM_OK;
}

int dqrm_emb_bwd_lsq_launches(const dqrm_table_set* set, const dqrm_batch* batch) {
    const int rc = check_set_batch(set, batch, "dqrm_emb_bwd_lsq_launches");
    if (rc) return rc;
    return batch->num_bags > 0 ? 2 : 0;
}

int dqrm_emb_fwd_pact(const dqrm_table_set* set, const dqrm_batch* batch, int bits, float* out, int64_t out_stride_t,
                      int64_t out_stride_b, void* stream) {
    const char* who = "dqrm_emb_fwd_pact";
    int rc = check_set_batch(set, batch, who);
    if (rc) return rc;
    if ((rc = check_bits(bits, who))) return rc;
    if ((rc = check_out(out, out_stride_t, out_stride_b, who))) return rc;
    if (batch->num_bags <= 0) return DQRM_OK;
    QFwdArgs a = fwd_args(set, batch, out, out_stride_t, out_stride_b);
    a.sc = (float)((1 << bits) - 1);
    return launch_fwd<MODE_PACT>(a, set->dim, (hipStream_t)stream);
}

int dqrm_emb_fwd_pact_launches(const dqrm_table_set* set, const dqrm_batch* batch) {
    const int rc = check_set_batch(set, batch, "dqrm_emb_fwd_pact_launches");
    if (rc) return rc;
    return batch->num_bags > 0 ? 1 : 0;
}

}  // extern "C"
