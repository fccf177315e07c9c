// dqrm_rowwise.hip — the row-wise PTQ formats of the reference's inference path, gfx950: the
// prepack and the one-table bag (dqrm_rowwise_prepack, dqrm_rowwise_bag), and the quantized
// model's embedding stage, every table's row-wise INT4 / INT8 bags in ONE launch
// (dqrm_rowwise_set_fwd).
//
// Reference (YangZhou08/Deep_Quantized_Recommendation_Model_DQRM @ 2024-10-24):
// DLRM_Net.quantize_embedding (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:683-700) prepacks every
// table with embedding_bag_{4bit,byte}_prepack and sets emb_l = None; apply_emb (:639-659) then
// calls embedding_bag_{4bit,byte}_rowwise_offsets table after table: 26 launches per batch. Here
// the packed tables are one slab u8 [R][row_bytes] (dqrm_rowwise_prepack's rows: 4-bit D/2 nibble
// bytes | fp16 scale | fp16 bias; byte D bytes | f32 scale | f32 bias), table t in rows
// [row_base[t], row_base[t] + num_rows[t]), and the grid is (bag chunks, tables).
//
// Arithmetic of the set kernel: k_rowwise_bag's (below), hence torch's: per lookup, in bag order,
// sc *= w, bi *= w when weights are given, acc[j] = fmaf(sc, q_j, acc[j] + bi) from acc = 0.
//
// Shape: G = D/8 lanes per bag, 8 dims per lane (two runs of 4: rowwise_load), dword and halfword
// loads (a 36-byte 4-bit row at D = 64 is only 4-byte aligned). The Criteo form (bag b = lookup
// b) is latency-bound on index -> row, like k_emb_fwd, and takes its remedy: UNR bags per lane
// group in flight, all index (and weight) loads first, then all row loads, unconditionally at
// clamped addresses, the values of invalid bags and indices dropped afterwards. The bag form keeps
// the sequential per-bag chain. No LDS. Measurements: DESIGN.md 5i.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dqrm_device.h"
#include "dqrm_internal.h"

namespace {

using dqrm_internal::grid_for;
using dqrm_internal::kMaxTables;  // as a dqrm_table_set
using dqrm_internal::set_error;

constexpr int kGridTarget = 8192;    // workgroups in all, as k_emb_fwd; grid-stride beyond

// ------------------------------------------------------------------------------------
// Row-wise PTQ formats of the reference's inference path:
//   prepack   torch.ops.quantized.embedding_bag_{4bit,byte}_prepack
//             (DLRM_Net.quantize_embedding, dlrm_s_pytorch_single_gpu_documentingp.py:689-704)
//   gather    torch.ops.quantized.embedding_bag_{4bit,byte}_rowwise_offsets, mode sum
//             (DLRM_Net.apply_emb, dlrm_s_pytorch_single_gpu_documentingp.py:648-663)
// Row layout (FBGEMM fused row-wise): 4-bit: D/2 nibble bytes (element 2j in the low
// nibble), fp16 scale, fp16 bias; 8-bit: D bytes, f32 scale, f32 bias. A row's scale and
// bias are read once per lookup next to its payload; G = D/8 lanes per row, 8 dims per lane.
// ------------------------------------------------------------------------------------
__host__ __device__ inline int rowwise_row_bytes(int bits, int D) { return bits == 4 ? D / 2 + 4 : D + 8; }

template <int G>
DQRM_INLINE float group_min(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, WAVE));
    return v;
}

template <int G>
DQRM_INLINE float group_fmax(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, WAVE));
    return v;
}

template <int BITS, int G>
__global__ void __launch_bounds__(256) k_rowwise_prepack(const float* __restrict__ W, int64_t n,
                                                         uint8_t* __restrict__ out) {
    constexpr int D = G * 8;
    constexpr int RB = BITS == 4 ? D / 2 + 4 : D + 8;
    const int lane = threadIdx.x % G;
    const int64_t rows_per_pass = (int64_t)gridDim.x * (256 / G);
    for (int64_t r = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; r < n; r += rows_per_pass) {
        const float4* src = reinterpret_cast<const float4*>(W + r * D) + lane * 2;
        const float4 a = src[0], b = src[1];
        float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        float mn = x[0], mx = x[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) { mn = fminf(mn, x[j]); mx = fmaxf(mx, x[j]); }
        mn = group_min<G>(mn);
        mx = group_fmax<G>(mx);
        uint8_t* orow = out + r * RB;
        if (BITS == 4) {  // FloatOrHalfToFusedNBitRowwiseQuantizedSBHalf, bit_rate 4
            const _Float16 mn16 = (_Float16)mn;  // round-to-nearest-even
            const float mnh = (float)mn16;
            const float range = mx - mnh;
            const float scale = range == 0.0f ? 1.0f : range / 15.0f;
            _Float16 s16 = (_Float16)scale;
            const float sh = (float)s16;
            float inv = sh == 0.0f ? 1.0f : 1.0f / sh;
            if (sh == 0.0f || isinf(inv)) { s16 = (_Float16)1.0f; inv = 1.0f; }
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float q = fminf(fmaxf(rintf((x[j] - mnh) * inv), 0.0f), 15.0f);
                word |= (uint32_t)q << (4 * j);
            }
            reinterpret_cast<uint32_t*>(orow)[lane] = word;
            if (lane == 0)
                reinterpret_cast<uint32_t*>(orow + D / 2)[0] =
                    (uint32_t)__builtin_bit_cast(uint16_t, s16) | ((uint32_t)__builtin_bit_cast(uint16_t, mn16) << 16);
        } else {          // FloatToFused8BitRowwiseQuantizedSBFloat
            const float range = mx - mn;
            const float scale = range / 255.0f;
            const float inv = 255.0f / (range + 1e-8f);
            uint2 words = make_uint2(0u, 0u);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float q = fminf(fmaxf(rintf((x[j] - mn) * inv), 0.0f), 255.0f);
                if (j < 4) words.x |= (uint32_t)q << (8 * j); else words.y |= (uint32_t)q << (8 * (j - 4));
            }
            reinterpret_cast<uint2*>(orow)[lane] = words;
            if (lane == 0) reinterpret_cast<uint2*>(orow + D)[0] = make_uint2(__float_as_uint(scale), __float_as_uint(mn));
        }
    }
}

// EmbeddingSpMDM(NBit) reference semantics, mode sum: per lookup, in bag order,
//   acc = fma(scale * w, q, acc + bias * w)     (w = per-sample weight, omitted when null)
template <int BITS, int G>
__global__ void __launch_bounds__(256) k_rowwise_bag(const uint8_t* __restrict__ packed, int64_t n,
                                                     const int64_t* __restrict__ idx, int64_t L,
                                                     const int64_t* __restrict__ off, int64_t B,
                                                     const float* __restrict__ psw, int last_offset,
                                                     float* __restrict__ out, uint32_t* __restrict__ err) {
    constexpr int D = G * 8;
    constexpr int RB = BITS == 4 ? D / 2 + 4 : D + 8;
    const int lane = threadIdx.x % G;
    const int64_t bags_per_pass = (int64_t)gridDim.x * (256 / G);
    for (int64_t b = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; b < B; b += bags_per_pass) {
        int64_t s0 = off[b], s1 = (b + 1 < B || last_offset) ? off[b + 1] : L;
        if (s0 < 0 || s1 > L || s1 < s0) {
            if (lane == 0) flag_error(err, DQRM_ERRF_OFFSET);
            s0 = s0 < 0 ? 0 : (s0 > L ? L : s0);
            s1 = s1 < s0 ? s0 : (s1 > L ? L : s1);
        }
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
        for (int64_t i = s0; i < s1; ++i) {
            const int64_t r = idx[i];
            if (r < 0 || r >= n) {
                if (lane == 0) flag_error(err, DQRM_ERRF_INDEX);
                continue;
            }
            const uint8_t* row = packed + r * RB;
            float sc, bi;
            uint32_t w0, w1 = 0;
            if (BITS == 4) {
                const uint32_t sb = *reinterpret_cast<const uint32_t*>(row + D / 2);
                sc = (float)__builtin_bit_cast(_Float16, (uint16_t)(sb & 0xFFFFu));
                bi = (float)__builtin_bit_cast(_Float16, (uint16_t)(sb >> 16));
                w0 = reinterpret_cast<const uint32_t*>(row)[lane];
            } else {
                const uint2 sb = *reinterpret_cast<const uint2*>(row + D);
                sc = __uint_as_float(sb.x);
                bi = __uint_as_float(sb.y);
                const uint2 w = reinterpret_cast<const uint2*>(row)[lane];
                w0 = w.x;
                w1 = w.y;
            }
            if (psw) {
                const float wt = psw[i];
                sc = sc * wt;
                bi = bi * wt;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float q = BITS == 4 ? (float)((w0 >> (4 * j)) & 15u)
                                          : (float)(((j < 4 ? w0 : w1) >> (8 * (j & 3))) & 255u);
                acc[j] = fmaf(sc, q, acc[j] + bi);
            }
        }
        float4* o = reinterpret_cast<float4*>(out + b * D) + lane * 2;
        o[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        o[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
}

// ------------------------------------------------------------------------------------
// Every table's bags in one launch (dqrm_rowwise_set_fwd)
// ------------------------------------------------------------------------------------
struct RowwiseSetArgs {
    const uint8_t* packed;
    const int64_t* meta;   // [2][T] row_base, num_rows
    uint32_t* err;
    const int64_t* idx;
    const int64_t* off;
    const int64_t* idx_base;
    const float* psw;      // nullable
    float* out;
    int64_t B;
    int64_t R;             // rows of the slab (>= 1)
    int64_t ost_t, ost_b;
    int T;
    int pool1;
    uint32_t wt;           // wt_stores() bits (WT_Y: out is stored write-through, st4_out)
};

// a lookup's 8 dims of this lane: sc / bi from the row's tail, q from its payload words
template <int BITS>
DQRM_INLINE void rowwise_acc(float (&acc)[8], float sc, float bi, uint32_t w0, uint32_t w1) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float q = BITS == 4 ? (float)((w0 >> (4 * j)) & 15u)
                                  : (float)(((j < 4 ? w0 : w1) >> (8 * (j & 3))) & 255u);
        acc[j] = fmaf(sc, q, acc[j] + bi);
    }
}

// A lane's share of a row: dims [4 lane, 4 lane + 4) and [D/2 + 4 lane, D/2 + 4 lane + 4), so that
// each of its two 16-B stores is contiguous with its neighbours' (G lanes write 16 G bytes in a
// row: whole 128-B lines from D = 64 on, which a write-through store needs). The 4-bit payload of
// those dims is two halfwords (w0 = low | high << 16), the byte payload two dwords; tl: the row's
// tail (fp16 scale | fp16 bias in one dword, or f32 scale, f32 bias). The row is 4-byte aligned.
template <int BITS, int D>
DQRM_INLINE void rowwise_load(const uint8_t* row, int lane, uint32_t (&tl)[BITS == 4 ? 1 : 2],
                              uint32_t (&pw)[BITS == 4 ? 1 : 2]) {
    const uint32_t* r32 = reinterpret_cast<const uint32_t*>(row);
    if constexpr (BITS == 4) {
        const uint16_t* r16 = reinterpret_cast<const uint16_t*>(row);
        tl[0] = r32[D / 8];
        pw[0] = (uint32_t)r16[lane] | ((uint32_t)r16[D / 8 + lane] << 16);
    } else {
        tl[0] = r32[D / 4];
        tl[1] = r32[D / 4 + 1];
        pw[0] = r32[lane];
        pw[1] = r32[D / 8 + lane];
    }
}

template <int BITS, int D>
DQRM_INLINE void rowwise_store(float* orow, int lane, const float (&acc)[8], bool wty) {
    st4_out(reinterpret_cast<float4*>(orow) + lane, make_float4(acc[0], acc[1], acc[2], acc[3]), wty);
    st4_out(reinterpret_cast<float4*>(orow + D / 2) + lane, make_float4(acc[4], acc[5], acc[6], acc[7]), wty);
}

template <int BITS, int D>
DQRM_INLINE void rowwise_tail(uint32_t t0, uint32_t t1, float* sc, float* bi) {
    if (BITS == 4) {
        *sc = (float)__builtin_bit_cast(_Float16, (uint16_t)(t0 & 0xFFFFu));
        *bi = (float)__builtin_bit_cast(_Float16, (uint16_t)(t0 >> 16));
    } else {
        *sc = __uint_as_float(t0);
        *bi = __uint_as_float(t1);
    }
}

template <int BITS, int G, int UNR>
__global__ void __launch_bounds__(256) k_rowwise_bag_set(RowwiseSetArgs a) {
    constexpr int D = G * 8;
    constexpr int RB = BITS == 4 ? D / 2 + 4 : D + 8;   // bytes per row, a multiple of 4
    constexpr int PW = BITS == 4 ? 1 : 2;               // payload dwords per lane
    constexpr int NG = 256 / G;                         // bags per workgroup pass and k
    // the table is blockIdx.y: every per-table value is wave-uniform
    const int t = blockIdx.y;
    const int64_t B = a.B;
    const int64_t rowbase = a.meta[t], nrows = a.meta[a.T + t];
    const int64_t ibase = a.pool1 ? (int64_t)t * B : a.idx_base[t];
    int64_t L = a.pool1 ? B : a.idx_base[t + 1] - ibase;
    if (L < 0) {  // a decreasing idx_base: no lookup of this table is read
        if (threadIdx.x == 0 && blockIdx.x == 0) flag_error(a.err, DQRM_ERRF_OFFSET);
        L = 0;
    }
    const int64_t* __restrict__ idx = a.idx + ibase;
    const float* __restrict__ psw = a.psw ? a.psw + ibase : nullptr;
    float* __restrict__ out = a.out + (int64_t)t * a.ost_t;
    const int lane = threadIdx.x % G;
    const int grp = threadIdx.x / G;
    const bool wty = (a.wt & WT_Y) != 0;
    const int64_t last_row = a.R - 1;

    if (a.pool1) {
        for (int64_t b0 = (int64_t)blockIdx.x * (NG * UNR); b0 < B; b0 += (int64_t)gridDim.x * (NG * UNR)) {
            // phase 1: the UNR bags' indices and weights (bag 0's for a bag past the end, dropped)
            int64_t rv[UNR];
            float wv[UNR];
#pragma unroll
            for (int k = 0; k < UNR; ++k) {
                const int64_t b = b0 + k * NG + grp;
                rv[k] = idx[b < B ? b : 0];
            }
            if (psw) {
#pragma unroll
                for (int k = 0; k < UNR; ++k) {
                    const int64_t b = b0 + k * NG + grp;
                    wv[k] = psw[b < B ? b : 0];
                }
            }
            // phase 2: the rows, at addresses clamped into the slab (row 0 of the table for an
            // invalid index; a table without rows loads nothing)
            bool ok[UNR];
            uint32_t tl[UNR][PW], pw[UNR][PW];
#pragma unroll
            for (int k = 0; k < UNR; ++k) {
                const int64_t b = b0 + k * NG + grp;
                ok[k] = rv[k] >= 0 && rv[k] < nrows;
                if (b < B && !ok[k] && lane == 0) flag_error(a.err, DQRM_ERRF_INDEX);
#pragma unroll
                for (int p = 0; p < PW; ++p) tl[k][p] = pw[k][p] = 0u;
            }
            if (nrows > 0) {
#pragma unroll
                for (int k = 0; k < UNR; ++k) {
                    int64_t gr = rowbase + (ok[k] ? rv[k] : 0);
                    gr = gr < 0 ? 0 : (gr > last_row ? last_row : gr);
                    rowwise_load<BITS, D>(a.packed + gr * RB, lane, tl[k], pw[k]);
                }
            }
            // phase 3: dequantize, then the stores together (st4_out: see k_emb_fwd)
            float acc[UNR][8];
#pragma unroll
            for (int k = 0; k < UNR; ++k) {
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[k][j] = 0.0f;
                if (!ok[k]) continue;
                float sc, bi;
                rowwise_tail<BITS, D>(tl[k][0], tl[k][PW - 1], &sc, &bi);
                if (psw) {
                    sc = sc * wv[k];
                    bi = bi * wv[k];
                }
                rowwise_acc<BITS>(acc[k], sc, bi, pw[k][0], pw[k][PW - 1]);
            }
#pragma unroll
            for (int k = 0; k < UNR; ++k) {
                const int64_t b = b0 + k * NG + grp;
                if (b >= B) continue;
                rowwise_store<BITS, D>(out + b * a.ost_b, lane, acc[k], wty);
            }
        }
        return;
    }

    // bag form: k_rowwise_bag's chain per bag
    const int64_t* __restrict__ off = a.off + (int64_t)t * B;
    for (int64_t b = (int64_t)blockIdx.x * NG + grp; b < B; b += (int64_t)gridDim.x * NG) {
        int64_t s0 = off[b], s1 = b + 1 < B ? off[b + 1] : L;
        if (s0 < 0 || s1 > L || s1 < s0) {
            if (lane == 0) flag_error(a.err, DQRM_ERRF_OFFSET);
            s0 = s0 < 0 ? 0 : (s0 > L ? L : s0);
            s1 = s1 < s0 ? s0 : (s1 > L ? L : s1);
        }
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
        for (int64_t i = s0; i < s1; ++i) {
            const int64_t r = idx[i];
            if (r < 0 || r >= nrows) {
                if (lane == 0) flag_error(a.err, DQRM_ERRF_INDEX);
                continue;
            }
            int64_t gr = rowbase + r;
            gr = gr < 0 ? 0 : (gr > last_row ? last_row : gr);
            uint32_t tl[PW], pw[PW];
            rowwise_load<BITS, D>(a.packed + gr * RB, lane, tl, pw);
            float sc, bi;
            rowwise_tail<BITS, D>(tl[0], tl[PW - 1], &sc, &bi);
            if (psw) {
                const float wt = psw[i];
                sc = sc * wt;
                bi = bi * wt;
            }
            rowwise_acc<BITS>(acc, sc, bi, pw[0], pw[PW - 1]);
        }
        rowwise_store<BITS, D>(out + b * a.ost_b, lane, acc, wty);
    }
}

template <int BITS, int G>
void launch_set(const RowwiseSetArgs& a, hipStream_t st) {
    // bags in flight per lane group (Criteo form). Measured, 26 tables, B = 16,384: 2 against 4
    // is 11.0 against 12.6 us at D = 16 and 29.1 against 29.3 us at D = 64
    constexpr int UNR = 2;
    const int64_t per_wg = a.pool1 ? (int64_t)(256 / G) * UNR : 256 / G;
    int64_t bx = (a.B + per_wg - 1) / per_wg;
    const int64_t cap = (kGridTarget + a.T - 1) / a.T;
    if (bx > cap) bx = cap;
    hipLaunchKernelGGL((k_rowwise_bag_set<BITS, G, UNR>), dim3((unsigned)bx, (unsigned)a.T), dim3(256), 0, st, a);
}

}  // namespace

int dqrm_internal::rowwise_set_check(const dqrm_rowwise_set* s, const dqrm_batch* batch, const char* who) {
    if (!s) return set_error(DQRM_E_INVALID, "%s: null row-wise set", who);
    if (s->num_tables <= 0 || s->num_tables > kMaxTables)
        return set_error(DQRM_E_INVALID, "%s: row-wise set: num_tables out of range (%d)", who, s->num_tables);
    if (s->bits != 4 && s->bits != 8)
        return set_error(DQRM_E_INVALID, "%s: row-wise set: bits must be 4 or 8 (got %d)", who, s->bits);
    const int D = s->dim;
    if (D != 8 && D != 16 && D != 32 && D != 64 && D != 128 && D != 256)
        return set_error(DQRM_E_INVALID, "%s: row-wise set: dim %d unsupported (8, 16, 32, 64, 128, 256)", who, D);
    if (s->total_rows < 1)
        return set_error(DQRM_E_INVALID, "%s: row-wise set: total_rows must be >= 1 (got %lld)", who,
                         (long long)s->total_rows);
    if (!s->packed || !s->meta || !s->err)
        return set_error(DQRM_E_INVALID, "%s: row-wise set: null packed / meta / err", who);
    if (((uintptr_t)s->packed) & 3)
        return set_error(DQRM_E_INVALID, "%s: row-wise set: packed must be 4-byte aligned", who);
    if (!batch) return DQRM_OK;
    if (batch->num_bags < 0) return set_error(DQRM_E_INVALID, "%s: negative num_bags", who);
    if (!batch->idx) return set_error(DQRM_E_INVALID, "%s: null batch idx", who);
    if (!(batch->flags & DQRM_BATCH_POOLING_ONE) && (!batch->off || !batch->idx_base))
        return set_error(DQRM_E_INVALID, "%s: a batch without DQRM_BATCH_POOLING_ONE needs off and idx_base", who);
    return DQRM_OK;
}

extern "C" {

#define DISPATCH_G(D, ...)                                                               \
    switch ((D) % 8 ? 0 : (D) / 8) {                                                     \
        case 1: { constexpr int G = 1; __VA_ARGS__; } break;                             \
        case 2: { constexpr int G = 2; __VA_ARGS__; } break;                             \
        case 4: { constexpr int G = 4; __VA_ARGS__; } break;                             \
        case 8: { constexpr int G = 8; __VA_ARGS__; } break;                             \
        case 16: { constexpr int G = 16; __VA_ARGS__; } break;                           \
        case 32: { constexpr int G = 32; __VA_ARGS__; } break;                           \
        default: return set_error(DQRM_E_INVALID, "dqrm rowwise: dim %d unsupported", (int)(D)); \
    }

size_t dqrm_rowwise_row_bytes(int bits, int dim) {
    if ((bits != 4 && bits != 8) || dim < 8 || (dim & 7)) return 0;
    return (size_t)rowwise_row_bytes(bits, dim);
}

int dqrm_rowwise_prepack(int bits, const float* W, int64_t num_rows, int dim, uint8_t* packed, void* stream) {
    if (bits != 4 && bits != 8) return set_error(DQRM_E_INVALID, "dqrm_rowwise_prepack: bits must be 4 or 8");
    if (!W || !packed || num_rows < 0) return set_error(DQRM_E_INVALID, "dqrm_rowwise_prepack: bad arguments");
    if (((uintptr_t)W) & 15) return set_error(DQRM_E_INVALID, "dqrm_rowwise_prepack: W must be 16-byte aligned");
    if (num_rows == 0) return DQRM_OK;
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_G(dim, {
        const int rows_per_wg = 256 / G;
        const int grid = grid_for(num_rows, rows_per_wg, 65536);
        if (bits == 4)
            hipLaunchKernelGGL((k_rowwise_prepack<4, G>), dim3(grid), dim3(256), 0, st, W, num_rows, packed);
        else
            hipLaunchKernelGGL((k_rowwise_prepack<8, G>), dim3(grid), dim3(256), 0, st, W, num_rows, packed);
    });
    LAUNCH_CHECK();
    return DQRM_OK;
}

int dqrm_rowwise_bag(int bits, const uint8_t* packed, int64_t num_rows, int dim, const int64_t* idx,
                     int64_t num_lookups, const int64_t* off, int64_t num_bags, int include_last_offset,
                     const float* per_sample_weights, float* out, uint32_t* err, void* stream) {
    if (bits != 4 && bits != 8) return set_error(DQRM_E_INVALID, "dqrm_rowwise_bag: bits must be 4 or 8");
    if (!packed || !off || !out || !err || (num_lookups > 0 && !idx) || num_rows < 0 || num_lookups < 0)
        return set_error(DQRM_E_INVALID, "dqrm_rowwise_bag: bad arguments");
    if (((uintptr_t)packed) & 3 || ((uintptr_t)out) & 15)
        return set_error(DQRM_E_INVALID, "dqrm_rowwise_bag: packed must be 4-B and out 16-B aligned");
    if (num_bags <= 0) return DQRM_OK;
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_G(dim, {
        const int bags_per_wg = 256 / G;
        const int grid = grid_for(num_bags, bags_per_wg, 65536);
        if (bits == 4)
            hipLaunchKernelGGL((k_rowwise_bag<4, G>), dim3(grid), dim3(256), 0, st, packed, num_rows, idx,
                               num_lookups, off, num_bags, per_sample_weights, include_last_offset, out, err);
        else
            hipLaunchKernelGGL((k_rowwise_bag<8, G>), dim3(grid), dim3(256), 0, st, packed, num_rows, idx,
                               num_lookups, off, num_bags, per_sample_weights, include_last_offset, out, err);
    });
    LAUNCH_CHECK();
    return DQRM_OK;
}

int dqrm_rowwise_set_fwd(const dqrm_rowwise_set* set, const dqrm_batch* batch, const float* per_sample_weights,
                         float* out, int64_t out_stride_t, int64_t out_stride_b, void* stream) {
    const char* who = "dqrm_rowwise_set_fwd";
    if (!batch) return set_error(DQRM_E_INVALID, "%s: null batch", who);
    int rc = dqrm_internal::rowwise_set_check(set, batch, who);
    if (rc) return rc;
    if (!out || (((uintptr_t)out) & 15) || (out_stride_t & 3) || (out_stride_b & 3))
        return set_error(DQRM_E_INVALID, "%s: out must be non-null, 16-B aligned, with strides %% 4 == 0", who);
    if (batch->num_bags == 0) return DQRM_OK;
    RowwiseSetArgs a;
    a.packed = set->packed; a.meta = set->meta; a.err = set->err;
    a.idx = batch->idx; a.off = batch->off; a.idx_base = batch->idx_base;
    a.psw = per_sample_weights; a.out = out;
    a.B = batch->num_bags; a.R = set->total_rows; a.ost_t = out_stride_t; a.ost_b = out_stride_b;
    a.T = set->num_tables;
    a.pool1 = (batch->flags & DQRM_BATCH_POOLING_ONE) != 0;
    a.wt = dqrm_internal::wt_stores(set->dim);  // the forwards' store policy, as dqrm_emb_fwd
    hipStream_t st = (hipStream_t)stream;
#define ROWWISE_SET_CASE(GV)                                                       \
    case GV * 8:                                                                   \
        if (set->bits == 4) launch_set<4, GV>(a, st); else launch_set<8, GV>(a, st); \
        break;
    switch (set->dim) {
        ROWWISE_SET_CASE(1)
        ROWWISE_SET_CASE(2)
        ROWWISE_SET_CASE(4)
        ROWWISE_SET_CASE(8)
        ROWWISE_SET_CASE(16)
        ROWWISE_SET_CASE(32)
        default: return set_error(DQRM_E_INVALID, "%s: dim %d unsupported", who, set->dim);
    }
#undef ROWWISE_SET_CASE
    LAUNCH_CHECK();
    return DQRM_OK;
}

}  // extern "C"
