// dqrm_exchange.hip — the N > 1 exchange step's quantize-pack (K5): the rank's coalesced
// gradient (slot workspace) -> its dense wire payload, with the table scales averaged over
// the ranks' all-gathered per-slot max|grad|. The whole stage: both kernels, the launcher and
// the dqrm_grad_quant_pack* exports.
//
// Reference: sgd_quantized_gradients_parallel_comm.py quantize_emb_grad :861-869
//   s_r = clamp(max|g|, 1e-8) / (2^(b-1) - 1)            (quant_utils.py:141-194)
//   dist.all_reduce(s, SUM); s.mul_(1/N)                  (:863-866; Gloo's one-element order)
//   q = clamp(round(1/s * g + 0), -2^(b-1), 2^(b-1) - 1)  (quant_utils.py:75-101, :322-346)
//
// Built for latency (the step is launch- and round-trip-bound, not HBM-bound: ~2.3 MB written
// per launch at TB): grid (T x SPLIT slots, CY chunks) of 256-thread workgroups, every wave
// derives the slot's payload offset and the table scale itself from lane-held loads (no LDS,
// no barrier), and each lane group keeps QU entries' loads in flight. Two dependent round
// trips per workgroup: the slot's uniform bases (scalar) with the counts and maxima, then the
// entries' rows and values.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dqrm_device.h"
#include "dqrm_internal.h"

namespace dqrm_internal {

// K5 quantize-pack of the N > 1 exchange (k_qpack): the rank's slot workspace ->
// its wire payload, the table scales averaged over the all-gathered per-slot maxima
// (dqrm_grad_quant_pack_strided's arguments, validated by the caller).
struct QuantPackArgs {
    int T;
    int D;
    const int64_t* ws_cap_base;  // [T*S+1]
    const int32_t* ws_rows;
    const float* ws_vals;
    const int32_t* ws_ucount;
    const float* absmax_all;     // [N][pitch], rank r's per-slot max|grad| at r*pitch + t*S + s
    int64_t am_pitch;
    int N;
    int bits;                    // 2..16 quantized, 32 = FP32 values
    const int64_t* cap_base;     // [T+1] payload capacity prefix
    int64_t cap_total;
    float* s_avg;                // [T]
    unsigned char* payload;
    uint32_t wt;                 // wt_stores() bits (WT_HAND: the payload values write-through)
};

}  // namespace dqrm_internal

namespace {

using dqrm_internal::QuantPackArgs;
using dqrm_internal::set_error;

constexpr int SPLIT = DQRM_TABLE_SPLIT;
constexpr int QP_TPB = 256;
constexpr int QP_QU = 4;  // entries per lane group in flight

template <int LPR>
__global__ void __launch_bounds__(QP_TPB) k_qpack(dqrm_internal::QuantPackArgs a) {
    constexpr int D = LPR * 4;
    constexpr int G = QP_TPB / LPR;         // lane groups (entries per pass)
    constexpr int E = G * QP_QU;            // entries per workgroup round
    const int k = blockIdx.x, t = k / SPLIT, s = k % SPLIT;
    const int tid = threadIdx.x, lane = tid % WAVE;
    const int N = a.N, bits = a.bits;
    const bool quant = bits >= 2 && bits <= 16;
    // round trip 1: the slot counts (lanes 0..7), rank r's slot maxima (lane r: 8 loads), and
    // the uniform bases (scalar loads)
    const int c_l = lane < SPLIT ? a.ws_ucount[t * SPLIT + lane] : 0;
    float am_l = 0.0f;
    if (quant && lane < N) {
        const float* p = a.absmax_all + (int64_t)lane * a.am_pitch + t * SPLIT;
        float x[SPLIT];
#pragma unroll
        for (int q = 0; q < SPLIT; ++q) x[q] = p[q];
#pragma unroll
        for (int q = 0; q < SPLIT; ++q) am_l = fmaxf(am_l, x[q]);
    }
    const int64_t ws0 = a.ws_cap_base[k], ws1 = a.ws_cap_base[k + 1];
    const int64_t cb0 = a.cap_base[t], cb1 = a.cap_base[t + 1];
    const PayloadLayout pl = payload_layout(a.T, a.cap_total, D, bits);
    const int scap = (int)(ws1 - ws0);  // the slot's workspace capacity
    const int sub = tid % LPR, grp = tid / LPR;
    const int u0 = (int)blockIdx.y * E + grp;
    const int ustride = (int)gridDim.y * E;
    // the first round of entries, issued before the counts arrive (indices clamped into the
    // slot's capacity; entries past the count are dropped below)
    float4 v[QP_QU];
    int32_t row[QP_QU];
    const float4* vals4 = reinterpret_cast<const float4*>(a.ws_vals);
#pragma unroll
    for (int h = 0; h < QP_QU; ++h) {
        int u = u0 + h * G;
        u = u < scap ? u : (scap > 0 ? scap - 1 : 0);
        const int64_t e = ws0 + u;
        v[h] = scap > 0 ? vals4[e * LPR + sub] : make_float4(0.f, 0.f, 0.f, 0.f);
        row[h] = scap > 0 ? a.ws_rows[e] : 0;
    }
    // the table's slot counts in slot order, clamped against its payload capacity (overflow
    // truncates the table), uniform in every wave
    const int cap = (int)(cb1 - cb0);
    int run = 0, pre = 0, my = 0;
#pragma unroll
    for (int q = 0; q < SPLIT; ++q) {
        int c = __builtin_amdgcn_readlane(c_l, q);
        c = c < cap - run ? c : cap - run;
        c = c < 0 ? 0 : c;
        if (q == s) { pre = run; my = c; }
        if (s == 0 && blockIdx.y == 0 && tid == q)  // the table's header counts
            reinterpret_cast<int32_t*>(a.payload)[t * SPLIT + q] = c;
        run += c;
    }
    // ranks' scales, summed in Gloo's one-element all_reduce order (descending rank), * 1/N
    float sv = 1.0f;
    if (quant) {
        const float s_l = sym_scale(am_l, bits);
        float acc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s_l), N - 1));
        for (int r = N - 2; r >= 0; --r)
            acc = acc + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s_l), r));
        sv = acc * (float)(1.0 / (double)N);
        if (s == 0 && blockIdx.y == 0 && tid == 0) a.s_avg[t] = sv;
    }
    const float rr = 1.0f / sv;
    const float qlo = -(float)(1 << (bits - 1)), qhi = (float)((1 << (bits - 1)) - 1);
    int32_t* prow = reinterpret_cast<int32_t*>(a.payload + pl.rows_off) + cb0 + pre;
    unsigned char* pval = a.payload + pl.vals_off + (cb0 + pre) * (int64_t)D * pl.elem;
    auto emit = [&](int u, float4 x, int32_t r) {
        if (sub == 0) prow[u] = r;
        if (!quant) {
            // (the quantized values are 4- or 8-B stores per lane: they stay plain)
            st4_out(reinterpret_cast<float4*>(pval + (int64_t)u * D * 4) + sub, x, (a.wt & WT_HAND) != 0);
            return;
        }
        const float q0 = fake_quant(x.x, rr, qlo, qhi), q1 = fake_quant(x.y, rr, qlo, qhi);
        const float q2 = fake_quant(x.z, rr, qlo, qhi), q3 = fake_quant(x.w, rr, qlo, qhi);
        if (pl.elem == 1) {
            const uint32_t pk = ((uint32_t)(uint8_t)(int8_t)(int)q0) | ((uint32_t)(uint8_t)(int8_t)(int)q1 << 8) |
                                ((uint32_t)(uint8_t)(int8_t)(int)q2 << 16) | ((uint32_t)(uint8_t)(int8_t)(int)q3 << 24);
            reinterpret_cast<uint32_t*>(pval + (int64_t)u * D)[sub] = pk;
        } else {
            uint2 pk;
            pk.x = ((uint32_t)(uint16_t)(int16_t)(int)q0) | ((uint32_t)(uint16_t)(int16_t)(int)q1 << 16);
            pk.y = ((uint32_t)(uint16_t)(int16_t)(int)q2) | ((uint32_t)(uint16_t)(int16_t)(int)q3 << 16);
            reinterpret_cast<uint2*>(pval + (int64_t)u * D * 2)[sub] = pk;
        }
    };
#pragma unroll
    for (int h = 0; h < QP_QU; ++h)
        if (u0 + h * G < my) emit(u0 + h * G, v[h], row[h]);
    // a slot beyond the grid's first round (crowded slot): the rest, grid-strided
    for (int ub = u0 + ustride; ub < my; ub += ustride) {
#pragma unroll
        for (int h = 0; h < QP_QU; ++h) {
            const int u = ub + h * G;
            if (u < my) {
                v[h] = vals4[(ws0 + u) * LPR + sub];
                row[h] = a.ws_rows[ws0 + u];
            }
        }
#pragma unroll
        for (int h = 0; h < QP_QU; ++h)
            if (ub + h * G < my) emit(ub + h * G, v[h], row[h]);
    }
}

hipError_t launch_quant_pack(const QuantPackArgs& a0, hipStream_t stream) {
    QuantPackArgs a = a0;
    a.wt = dqrm_internal::wt_stores(a.D);
    // chunks per slot: the payload capacity spread evenly over the slots (a Criteo batch's
    // rows land roughly evenly in a table's row ranges), at least 1, at most 16
    const int64_t slots = (int64_t)a.T * SPLIT;
    auto chunks = [&](int lpr) {
        const int64_t e = (int64_t)(QP_TPB / lpr) * QP_QU;
        int64_t cy = (a.cap_total + slots * e - 1) / (slots * e);
        return (unsigned)(cy < 1 ? 1 : (cy > 16 ? 16 : cy));
    };
    const dim3 grid((unsigned)slots, 1);
    switch (a.D) {
#define QP_CASE(Dd)                                                                               \
    case Dd: {                                                                                    \
        constexpr int LPR = Dd / 4;                                                               \
        hipLaunchKernelGGL(k_qpack<LPR>, dim3(grid.x, chunks(LPR)), dim3(QP_TPB), 0, stream, a); \
    } break;
        QP_CASE(4) QP_CASE(8) QP_CASE(16) QP_CASE(32) QP_CASE(64) QP_CASE(128) QP_CASE(256)
#undef QP_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// The earlier K5 (DQRM_QPACK=legacy, A/B) and the ranking range's pack, which has no other kernel.
// ------------------------------------------------------------------------------------
// One workgroup per (table, slot): the table's 8 slot counts are clamped in slot order
// against the table's payload capacity (overflow truncates the table), the N ranks'
// per-slot max|grad| are staged in LDS and averaged in Gloo's order, then LPR lanes per
// entry quantize and store the slot's entries at their dense payload position. Workgroup
// (t, 0) also writes the table's header counts and s_avg[t].
template <int LPR>
__global__ void __launch_bounds__(512) k_quant_pack(int T, const int64_t* __restrict__ ws_cap_base,
                                                    int64_t ws_cap_total, const int32_t* __restrict__ ws_rows,
                                                    const float* __restrict__ ws_vals,
                                                    const int32_t* __restrict__ ws_ucount,
                                                    const float* __restrict__ absmax_all, int64_t am_pitch,
                                                    int N, int bits,
                                                    const int64_t* __restrict__ cap_base, int64_t cap_total,
                                                    float* __restrict__ s_avg, unsigned char* __restrict__ payload,
                                                    const int32_t* __restrict__ tbits,
                                                    const float* __restrict__ tscale) {
    __shared__ int s_cnt[SPLIT];
    __shared__ float s_am[64 * SPLIT];
    __shared__ int s_pre, s_my;
    __shared__ float s_sc;
    (void)ws_cap_total;
    const int k = blockIdx.x, t = k / SPLIT, s = k % SPLIT;
    const int D = LPR * 4;
    const PayloadLayout pl = payload_layout(T, cap_total, D, bits);
    // ranking range (tbits != NULL): per-table bit width and scale; 0 / 32-bit tables send
    // nothing (grad_update_parallel_comm skips them, s_q_g_p_c.py:280-289)
    const int tb = tbits ? tbits[t] : bits;
    const bool ranked = tbits != nullptr;
    const bool send = !ranked || (tb >= 2 && tb <= 8);
    const bool quant = !ranked && bits >= 2 && bits <= 16;
    if (threadIdx.x < SPLIT) s_cnt[threadIdx.x] = send ? ws_ucount[t * SPLIT + threadIdx.x] : 0;
    if (quant)
        for (int j = threadIdx.x; j < N * SPLIT; j += blockDim.x)
            s_am[j] = absmax_all[(int64_t)(j / SPLIT) * am_pitch + t * SPLIT + (j % SPLIT)];
    __syncthreads();
    if (threadIdx.x == 0) {
        const int cap = (int)(cap_base[t + 1] - cap_base[t]);
        int run = 0;
        for (int ss = 0; ss < SPLIT; ++ss) {
            int c = s_cnt[ss];
            c = c < cap - run ? c : cap - run;  // overflow: the table's payload is truncated
            c = c < 0 ? 0 : c;
            if (ss == s) { s_pre = run; s_my = c; }
            if (s == 0) reinterpret_cast<int32_t*>(payload)[t * SPLIT + ss] = c;
            run += c;
        }
        if (quant) {  // rank scales, then Gloo's one-element all_reduce order
            const float inv_n = (float)(1.0 / (double)N);
            float acc = 0.0f;
            for (int r = N - 1; r >= 0; --r) {
                float am = 0.0f;
                for (int ss = 0; ss < SPLIT; ++ss) am = fmaxf(am, s_am[r * SPLIT + ss]);
                const float sr = sym_scale(am, bits);
                acc = r == N - 1 ? sr : acc + sr;
            }
            const float sv = acc * inv_n;
            s_sc = sv;
            if (s == 0) s_avg[t] = sv;
        }
    }
    __syncthreads();
    const int cnt = s_my;
    const int64_t src0 = ws_cap_base[k], dst0 = cap_base[t] + s_pre;
    const bool qv = quant || (ranked && send);  // values are quantized
    const float rr = quant ? 1.0f / s_sc : (qv ? 1.0f / tscale[t] : 0.0f);
    const int lane = threadIdx.x % LPR;
    constexpr int QU = 4;                 // entries in flight per lane group
    constexpr int EPI = 512 / LPR;        // lane groups per workgroup
    const int qb = ranked ? (send ? tb : 2) : bits;
    const float qlo = -(float)(1 << (qb - 1)), qhi = (float)((1 << (qb - 1)) - 1);
    for (int u0 = threadIdx.x / LPR; u0 < cnt; u0 += QU * EPI) {
        float4 v[QU];
        int32_t row[QU];
#pragma unroll
        for (int h = 0; h < QU; ++h) {  // QU entries' loads in flight
            const int u = u0 + h * EPI;
            if (u < cnt) {
                v[h] = reinterpret_cast<const float4*>(ws_vals + (src0 + u) * D)[lane];
                row[h] = ws_rows[src0 + u];
            }
        }
#pragma unroll
        for (int h = 0; h < QU; ++h) {
            const int u = u0 + h * EPI;
            if (u >= cnt) continue;
            const int64_t q = dst0 + u;  // dense payload entry
            if (lane == 0) reinterpret_cast<int32_t*>(payload + pl.rows_off)[q] = row[h];
            if (!qv) {
                reinterpret_cast<float4*>(payload + pl.vals_off + q * D * 4)[lane] = v[h];
                continue;
            }
            const float q0 = fake_quant(v[h].x, rr, qlo, qhi), q1 = fake_quant(v[h].y, rr, qlo, qhi);
            const float q2 = fake_quant(v[h].z, rr, qlo, qhi), q3 = fake_quant(v[h].w, rr, qlo, qhi);
            if (pl.elem == 1) {
                uint32_t pk = ((uint32_t)(uint8_t)(int8_t)(int)q0) | ((uint32_t)(uint8_t)(int8_t)(int)q1 << 8) |
                              ((uint32_t)(uint8_t)(int8_t)(int)q2 << 16) | ((uint32_t)(uint8_t)(int8_t)(int)q3 << 24);
                reinterpret_cast<uint32_t*>(payload + pl.vals_off + q * D)[lane] = pk;
            } else {
                uint2 pk;
                pk.x = ((uint32_t)(uint16_t)(int16_t)(int)q0) | ((uint32_t)(uint16_t)(int16_t)(int)q1 << 16);
                pk.y = ((uint32_t)(uint16_t)(int16_t)(int)q2) | ((uint32_t)(uint16_t)(int16_t)(int)q3 << 16);
                reinterpret_cast<uint2*>(payload + pl.vals_off + q * D * 2)[lane] = pk;
            }
        }
    }
}

}  // namespace

extern "C" {

int dqrm_grad_quant_pack_strided(int num_tables, int dim, const int64_t* ws_cap_base, int64_t ws_cap_total,
                                 const int32_t* ws_rows, const float* ws_vals, const int32_t* ws_ucount,
                                 const float* absmax_all, int64_t absmax_pitch, int num_ranks, int grad_bits,
                                 const int64_t* cap_base, int64_t cap_total, float* s_avg, void* payload,
                                 void* stream) {
    if (num_tables <= 0 || num_tables > dqrm_internal::kMaxTables || num_ranks <= 0 || num_ranks > 64)
        return set_error(DQRM_E_INVALID, "%s: bad num_tables/num_ranks", "dqrm_grad_quant_pack");
    if (!(grad_bits == 32 || (grad_bits >= 2 && grad_bits <= 16)))
        return set_error(DQRM_E_INVALID, "%s: grad bits %d unsupported", "dqrm_grad_quant_pack", grad_bits);
    if (!ws_cap_base || !ws_rows || !ws_vals || !ws_ucount || !cap_base || !payload ||
        (grad_bits != 32 && (!absmax_all || !s_avg)))
        return set_error(DQRM_E_INVALID, "%s: null pointer", "dqrm_grad_quant_pack");
    if (num_ranks > 1 && absmax_pitch < (int64_t)num_tables * SPLIT)
        return set_error(DQRM_E_INVALID, "%s: absmax pitch %lld < %d", "dqrm_grad_quant_pack",
                         (long long)absmax_pitch, num_tables * SPLIT);
    if (((uintptr_t)payload) & 15)
        return set_error(DQRM_E_INVALID, "%s: payload must be 16-B aligned", "dqrm_grad_quant_pack");
    hipStream_t st = (hipStream_t)stream;
    if (!dqrm_internal::env_qpack_legacy()) {  // (legacy: the one-workgroup-per-slot kernel, A/B)
        QuantPackArgs q{num_tables, dim, ws_cap_base, ws_rows, ws_vals, ws_ucount, absmax_all, absmax_pitch,
                        num_ranks, grad_bits, cap_base, cap_total, s_avg, (unsigned char*)payload};
        DQRM_HIP_TRY(launch_quant_pack(q, st));
        return DQRM_OK;
    }
    DISPATCH_LPR(dim, {
        hipLaunchKernelGGL(k_quant_pack<LPR>, dim3(num_tables * SPLIT), dim3(512), 0, st,
                           num_tables, ws_cap_base, ws_cap_total, ws_rows, ws_vals, ws_ucount, absmax_all,
                           absmax_pitch, num_ranks, grad_bits, cap_base, cap_total, s_avg, (unsigned char*)payload,
                           (const int32_t*)nullptr, (const float*)nullptr);
    });
    LAUNCH_CHECK();
    return DQRM_OK;
}

int dqrm_grad_quant_pack(int num_tables, int dim, const int64_t* ws_cap_base, int64_t ws_cap_total,
                         const int32_t* ws_rows, const float* ws_vals, const int32_t* ws_ucount,
                         const float* absmax_all, int num_ranks, int grad_bits, const int64_t* cap_base,
                         int64_t cap_total, float* s_avg, void* payload, void* stream) {
    return dqrm_grad_quant_pack_strided(num_tables, dim, ws_cap_base, ws_cap_total, ws_rows, ws_vals, ws_ucount,
                                        absmax_all, (int64_t)num_tables * SPLIT, num_ranks, grad_bits, cap_base,
                                        cap_total, s_avg, payload, stream);
}

int dqrm_grad_quant_pack_ranked(int num_tables, int dim, const int64_t* ws_cap_base, int64_t ws_cap_total,
                                const int32_t* ws_rows, const float* ws_vals, const int32_t* ws_ucount,
                                const int32_t* table_bits, const float* table_scale, const int64_t* cap_base,
                                int64_t cap_total, void* payload, void* stream) {
    if (num_tables <= 0 || num_tables > dqrm_internal::kMaxTables)
        return set_error(DQRM_E_INVALID, "%s: bad num_tables", "dqrm_grad_quant_pack_ranked");
    if (!ws_cap_base || !ws_rows || !ws_vals || !ws_ucount || !table_bits || !table_scale || !cap_base || !payload)
        return set_error(DQRM_E_INVALID, "%s: null pointer", "dqrm_grad_quant_pack_ranked");
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_LPR(dim, {
        hipLaunchKernelGGL(k_quant_pack<LPR>, dim3(num_tables * SPLIT), dim3(512), 0, st,
                           num_tables, ws_cap_base, ws_cap_total, ws_rows, ws_vals, ws_ucount,
                           (const float*)nullptr, (int64_t)0, 1, 8, cap_base, cap_total, (float*)nullptr,
                           (unsigned char*)payload, table_bits, table_scale);
    });
    LAUNCH_CHECK();
    return DQRM_OK;
}

}  // extern "C"
