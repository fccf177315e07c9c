// dqrm_linear.hip — QuantLinear (fake-quantized MLP layer) forward / backward on the f32-input
// MFMA, gfx950.
//
// Reference (YangZhou08/Deep_Quantized_Recommendation_Model_DQRM @ 2024-10-24,
// quantization_supp/):
//   QuantLinear.forward              quant_modules_not_quantize_grad.py:105-211
//   symmetric_linear_quantization_params   quant_utils.py:196-220
//   linear_quantize                  quant_utils.py:75-101     round(1/s * x + 0)
//   SymmetricQuantFunction           quant_utils.py:316-363    clamp forward, grad / s backward (STE)
//
// Entry points: dqrm_linear_wquant (scale + integer weights and bias), dqrm_linear_fwd_act and
// dqrm_linear_bwd_act (the layer with the MLP's ReLU / Sigmoid fused in), and dqrm_linear_fwd /
// _bwd, which are those two without an activation; dqrm_linear_wquant_qact / _fwd_qact /
// _bwd_qact are the integer-activation branch (quantize_activation with a previous activation
// scale, q_m_n_q_g.py:150-161, :193-196) on the same kernels. All three matrix products go through ONE
// LDS-tiled kernel template on
// v_mfma_f32_16x16x4_f32, which is bit for bit an f32 fmaf chain in ascending k with one
// rounding per product: every output element is
//     acc = 0;  for k = 0..K-1: acc = fmaf(a[k], b[k], acc)
// whatever the tile shape, the grid or the other rows of the batch. No atomics, no split
// reductions: the result is a pure function of the operands. Ragged tile edges are zero-filled
// (fmaf(0, 0, acc) == acc up to the sign of an exact zero).
//
// The 16x16x4 shape is chosen over 32x32x2 for its dependent-accumulator latency: these layers
// are small (B = 128..2048, features 13..512) and a tile's time is its K chain, 40 cycles per
// four k against 64 cycles per two. Workgroup = 4 waves as 2 x 2; a wave owns WT x WT tiles of
// 16 x 16 (WT = 1: 32 x 32 outputs per workgroup, for grids that would not fill the chip
// otherwise; WT = 2: 64 x 64, half the staging traffic per FLOP). An LDS stage holds BK = 64 / WT
// k (a grid of few workgroups has nothing else to cover a global load's latency with, so a stage
// is as deep as eight floats per thread and operand allow), two LDS buffers, the next stage's
// global loads in flight during the MFMAs.
//
// Compiled with -ffp-contract=off: `g = dy * s`, `(acc + bi) * s` and `acc / s` are separately
// rounded operations, as the reference's autograd graph performs them; so are the activation's
// `1 / (1 + expf(-z))` and its derivative `(dy * (1 - y)) * y`.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/dqrm.h"
#include "dqrm_internal.h"
#include "dqrm_device.h"

namespace {

using dqrm_internal::set_error;

constexpr int LWG = 256;            // threads per workgroup (4 waves, 2 x 2)
constexpr int QWG = 256;            // wquant: threads per workgroup
constexpr int QRPW = QWG / WAVE;    // wquant: weight rows per workgroup (one per wave)
constexpr int AWG = 1024;           // per-tensor abs-max: one workgroup

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------ wquant
struct QuantArgs {
    int out, in;
    const float* W;
    const float* b;
    float* wi;
    float* bi;
    float* scale;
    float n;              // 2^(weight_bit-1) - 1
    float wlo, whi;       // weight clamp
    float blo, bhi;       // bias clamp
    const float* prev;    // QA: the previous activation scale p, one float
    float* cos;           // QA: out_scale[o] = scale[o] * p, [out] or [1]
};

// QA (the integer-activation branch, q_m_n_q_g.py:150-154): the bias is quantized with
// cos = s * p in place of s, and cos is stored at cos[cos_at] (cos_at < 0: by another row).
template <bool QA>
__device__ __forceinline__ void quant_bias(const QuantArgs& a, int o, float s, float rcp, int cos_at) {
    if (QA) {
        const float c = s * a.prev[0];
        if (cos_at >= 0) a.cos[cos_at] = c;
        a.bi[o] = fake_quant(a.b[o], 1.0f / c, a.blo, a.bhi);
    } else {
        a.bi[o] = fake_quant(a.b[o], rcp, a.blo, a.bhi);
    }
}

// per_channel: one wave per weight row: s[o] = clamp(max(|min_k W|, |max_k W|), 1e-8) / n
// (== max_k |W| for finite W), the row's integers, and the row's bias integer.
template <bool QA>
__global__ void __launch_bounds__(QWG) k_wquant_rows(QuantArgs a) {
    const int o = blockIdx.x * QRPW + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (o >= a.out) return;
    const float* __restrict__ w = a.W + (int64_t)o * a.in;
    float* __restrict__ wi = a.wi + (int64_t)o * a.in;
    float m = 0.0f;
    for (int k = lane; k < a.in; k += WAVE) m = fmaxf(m, fabsf(w[k]));
    m = wave_max(m);
    const float s = fmaxf(m, 1e-8f) / a.n;
    const float rcp = 1.0f / s;
    for (int k = lane; k < a.in; k += WAVE) wi[k] = fake_quant(w[k], rcp, a.wlo, a.whi);
    if (lane == 0) {
        a.scale[o] = s;
        quant_bias<QA>(a, o, s, rcp, o);
    }
}

// per tensor, launch 1: one workgroup, scale[0] = clamp(max |W|, 1e-8) / n (a maximum does not
// depend on the order it is taken in)
__global__ void __launch_bounds__(AWG) k_wquant_absmax(QuantArgs a) {
    __shared__ float part[AWG / WAVE];
    const int64_t total = (int64_t)a.out * a.in;
    float m = 0.0f;
    for (int64_t e = threadIdx.x; e < total; e += AWG) m = fmaxf(m, fabsf(a.W[e]));
    m = wave_max(m);
    if (threadIdx.x % WAVE == 0) part[threadIdx.x / WAVE] = m;
    __syncthreads();
    if (threadIdx.x < WAVE) {
        m = threadIdx.x < AWG / WAVE ? part[threadIdx.x] : 0.0f;
        m = wave_max(m);
        if (threadIdx.x == 0) a.scale[0] = fmaxf(m, 1e-8f) / a.n;
    }
}

// per tensor, launch 2: the integers of every row and bias with scale[0]
template <bool QA>
__global__ void __launch_bounds__(QWG) k_wquant_tensor(QuantArgs a) {
    const int o = blockIdx.x * QRPW + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (o >= a.out) return;
    const float* __restrict__ w = a.W + (int64_t)o * a.in;
    float* __restrict__ wi = a.wi + (int64_t)o * a.in;
    const float s = a.scale[0];
    const float rcp = 1.0f / s;
    for (int k = lane; k < a.in; k += WAVE) wi[k] = fake_quant(w[k], rcp, a.wlo, a.whi);
    if (lane == 0) quant_bias<QA>(a, o, s, rcp, o == 0 ? 0 : -1);
}

// ------------------------------------------------------------------------------ the GEMM
// C[m][n] = epilogue(chain over k of A(m, k) * B(k, n)), C row-major [M][N].
//   FWD (NT): A(m,k) = x[m][k]            B(k,n) = w[n][k]    C = (acc + bias[n]) * s[n]
//   DX  (NN): A(m,k) = dy[m][k] * s[k]    B(k,n) = w[k][n]    C = acc
//   DW  (TN): A(m,k) = dy[k][m] * s[m]    B(k,n) = x[k][n]    C = acc / s[m]
//             and, in the workgroups of the first tile column, db[m] = (chain over k of A(m,k)) / s[m]
// s == nullptr: s = 1 (full precision: multiplying or dividing by 1 is exact). s_stride = 0:
// one scale for the whole tensor.
// ACT (DQRM_ACT_*), the activation that follows the layer in create_mlp: FWD stores act(C); DX
// and DW read, beside each dy element, the forward's output y at the same address, and dy above
// stands for d = dy * act'(y) (RELU: y <= 0 ? 0 : dy; SIGMOID: (dy * (1 - y)) * y), formed before
// the scale is applied. db sums the staged A tile and so follows.
// QA (the integer-activation branch, q_m_n_q_g.py:158-161, :193-196), p = prev[0], s = cos
// (out_scale), ws = the weight's scale:
//   FWD: A(m,k) = x[m][k] / p             C = rintf(acc + bias[n]) * cos[n]
//   DX:  A(m,k) = dy[m][k] * cos[k]       C = acc / p
//   DW:  A(m,k) = dy[k][m] * cos[m]       B(k,n) = x[k][n] / p    C = acc / ws[m]
//        db[m] = (chain over k of A(m,k)) / cos[m]
// The division by p is formed on load into LDS, like the STE's scale.
enum { FWD = 0, DX = 1, DW = 2 };

struct GemmArgs {
    int M, N, K;
    const float* A;
    const float* B;
    float* C;
    const float* s;
    int s_stride;
    const float* bias;  // FWD
    float* db;          // DW
    const float* Y;     // DX / DW with an activation: the forward's output, laid out as A
    const float* prev;  // QA: p
    const float* ws;    // QA, DW: the weight's scale (s_stride as s)
};

// Stage a BK x BMN operand tile into LDS as dst[k][r] (zero outside the matrix).
// KCONTIG: element (r, k) at src[r * ld + k], lanes run along k; else at src[k * ld + r], lanes
// run along r. SC: 1 = times s[k], 2 = times s[r] (the STE's g = dy * s, formed on load);
// 3 = divided by the one p store() is given (the integer activation x / p).
// ACT != NONE: a second register stream yv[] holds the forward's output at v[]'s addresses and
// store() turns v into v * act'(yv) before the scale.
template <int BMN, int BK, int LDS_LD, bool KCONTIG, int SC, int ACT>
struct Stage {
    static constexpr int PER = BK * BMN / LWG;
    float v[PER];
    float sv[SC == 1 || SC == 2 ? PER : 1];
    float yv[ACT != DQRM_ACT_NONE ? PER : 1];
    uint32_t ok;  // bit i: element i lies inside the matrix

    __device__ __forceinline__ static void pos(int e, int& kk, int& r) {
        if (KCONTIG) {
            kk = e % BK;
            r = e / BK;
        } else {
            r = e % BMN;
            kk = e / BMN;
        }
    }

    // Issues the stage's loads and nothing that waits for them: every element is loaded
    // unconditionally (from element (0, 0) when it lies outside the matrix) and the activation's
    // derivative and the scale are applied in store(), so the loads stay in flight during the
    // MFMAs between the two calls.
    __device__ __forceinline__ void load(const float* __restrict__ src, int64_t ld, int r0, int k0, int R, int K,
                                         const float* __restrict__ s, int s_stride,
                                         const float* __restrict__ ysrc) {
        ok = 0;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            int kk, r;
            pos((int)threadIdx.x + i * LWG, kk, r);
            const bool in = r0 + r < R && k0 + kk < K;
            const int gr = in ? r0 + r : 0, gk = in ? k0 + kk : 0;
            ok |= (uint32_t)in << i;
            const int64_t at = KCONTIG ? (int64_t)gr * ld + gk : (int64_t)gk * ld + gr;
            v[i] = src[at];
            if (ACT != DQRM_ACT_NONE) yv[i] = ysrc[at];
            if (SC == 1 || SC == 2) sv[i] = s != nullptr ? s[(int64_t)(SC == 1 ? gk : gr) * s_stride] : 1.0f;
        }
    }

    __device__ __forceinline__ void store(float (*dst)[LDS_LD], float p) const {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            int kk, r;
            pos((int)threadIdx.x + i * LWG, kk, r);
            float x = v[i];
            if (ACT == DQRM_ACT_RELU) x = yv[i] <= 0.0f ? 0.0f : x;
            if (ACT == DQRM_ACT_SIGMOID) x = (x * (1.0f - yv[i])) * yv[i];
            if (SC == 1 || SC == 2) x = x * sv[i];
            if (SC == 3) x = x / p;
            dst[kk][r] = (ok >> i) & 1u ? x : 0.0f;
        }
    }
};

template <int WT, int MODE, int ACT, bool QA>
__global__ void __launch_bounds__(LWG) k_linear_gemm(GemmArgs g) {
    constexpr int BT = 32 * WT;      // workgroup tile edge
    constexpr int BK = 64 / WT;      // k per LDS stage (16 or 8 MFMA k-steps; 8 floats per thread and operand)
    // row stride == 17 (mod 32) words: the k-major stores of a k-contiguous operand and the
    // MFMA operand reads (16 consecutive r for 4 k) both spread over the banks
    constexpr int LD = BT + 17;
    constexpr bool A_KC = MODE != DW;
    constexpr bool B_KC = MODE == FWD;
    constexpr int A_SC = MODE == DX ? 1 : (MODE == DW ? 2 : (QA ? 3 : 0));
    constexpr int B_SC = QA && MODE == DW ? 3 : 0;
    constexpr int A_ACT = MODE == FWD ? DQRM_ACT_NONE : ACT;  // FWD applies it in the epilogue
    __shared__ float As[2][BK][LD];
    __shared__ float Bs[2][BK][LD];

    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    const int m0 = blockIdx.y * BT, n0 = blockIdx.x * BT;
    const int wm = (wave >> 1) * 16 * WT, wn = (wave & 1) * 16 * WT;  // the wave's corner in the tile
    const int lr = lane & 15, lk = lane >> 4;
    const int64_t lda = MODE == DW ? g.M : g.K;   // A's row pitch in memory
    const int64_t ldb = MODE == FWD ? g.K : g.N;

    f32x4 acc[WT][WT];
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const bool do_db = MODE == DW && blockIdx.x == 0 && tid < BT;
    float dbacc = 0.0f;

    Stage<BT, BK, LD, A_KC, A_SC, A_ACT> sa;
    Stage<BT, BK, LD, B_KC, B_SC, DQRM_ACT_NONE> sb;
    const int T = (g.K + BK - 1) / BK;
    const float p = QA ? g.prev[0] : 1.0f;
    sa.load(g.A, lda, m0, 0, g.M, g.K, g.s, g.s_stride, g.Y);
    sb.load(g.B, ldb, n0, 0, g.N, g.K, nullptr, 0, nullptr);
    sa.store(As[0], p);
    sb.store(Bs[0], p);
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const int cur = t & 1;
        if (t + 1 < T) {  // in flight during the MFMAs below
            sa.load(g.A, lda, m0, (t + 1) * BK, g.M, g.K, g.s, g.s_stride, g.Y);
            sb.load(g.B, ldb, n0, (t + 1) * BK, g.N, g.K, nullptr, 0, nullptr);
        }
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) {
            float a[WT], b[WT];
#pragma unroll
            for (int i = 0; i < WT; ++i) a[i] = As[cur][ks * 4 + lk][wm + i * 16 + lr];
#pragma unroll
            for (int j = 0; j < WT; ++j) b[j] = Bs[cur][ks * 4 + lk][wn + j * 16 + lr];
#pragma unroll
            for (int i = 0; i < WT; ++i)
#pragma unroll
                for (int j = 0; j < WT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (do_db) {
#pragma unroll
            for (int kk = 0; kk < BK; ++kk) dbacc = dbacc + As[cur][kk][tid];
        }
        if (t + 1 < T) {
            sa.store(As[cur ^ 1], p);
            sb.store(Bs[cur ^ 1], p);
        }
        __syncthreads();
    }

    // C/D map of the 16x16 tile: column = lane & 15, row = 4 * (lane >> 4) + register
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j) {
            const int n = n0 + wn + j * 16 + lr;
            if (n >= g.N) continue;
            float sn = 1.0f, bn = 0.0f;
            if (MODE == FWD) {
                if (g.s != nullptr) sn = g.s[(int64_t)n * g.s_stride];
                bn = g.bias[n];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + i * 16 + lk * 4 + r;
                if (m >= g.M) continue;
                float c = acc[i][j][r];
                if (MODE == FWD) {
                    c = QA ? rintf(c + bn) * sn : (c + bn) * sn;
                    if (ACT == DQRM_ACT_RELU) c = c <= 0.0f ? 0.0f : c;  // keeps a NaN, -0 becomes +0
                    if (ACT == DQRM_ACT_SIGMOID) c = 1.0f / (1.0f + expf(-c));
                }
                if (MODE == DX && QA) c = c / p;
                if (MODE == DW && QA) c = c / g.ws[(int64_t)m * g.s_stride];
                if (MODE == DW && !QA && g.s != nullptr) c = c / g.s[(int64_t)m * g.s_stride];
                g.C[(int64_t)m * g.N + n] = c;
            }
        }
    if (do_db) {
        const int m = m0 + tid;
        if (m < g.M) g.db[m] = g.s != nullptr ? dbacc / g.s[(int64_t)m * g.s_stride] : dbacc;
    }
}

// Tile choice from the shape alone: 32 x 32 workgroup tiles until they number four per CU of
// a 256-CU part, 64 x 64 beyond. The bits do not depend on it.
constexpr int64_t kSmallTileMax = 1024;

template <int MODE, int ACT, bool QA>
int launch_gemm_act(const GemmArgs& g, hipStream_t st, const char* what) {
    const int64_t bm = (g.M + 31) / 32, bn = (g.N + 31) / 32;
    if (bm * bn < kSmallTileMax) {
        if (bm > 65535) return set_error(DQRM_E_CAPACITY, "%s: more than 65535 row tiles", what);
        hipLaunchKernelGGL((k_linear_gemm<1, MODE, ACT, QA>), dim3((unsigned)bn, (unsigned)bm), dim3(LWG), 0, st, g);
    } else {
        const int64_t bm2 = (g.M + 63) / 64, bn2 = (g.N + 63) / 64;
        if (bm2 > 65535) return set_error(DQRM_E_CAPACITY, "%s: more than 65535 row tiles", what);
        hipLaunchKernelGGL((k_linear_gemm<2, MODE, ACT, QA>), dim3((unsigned)bn2, (unsigned)bm2), dim3(LWG), 0, st, g);
    }
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

template <int MODE, bool QA = false>
int launch_gemm(const GemmArgs& g, int act, hipStream_t st, const char* what) {
    switch (act) {
        case DQRM_ACT_RELU: return launch_gemm_act<MODE, DQRM_ACT_RELU, QA>(g, st, what);
        case DQRM_ACT_SIGMOID: return launch_gemm_act<MODE, DQRM_ACT_SIGMOID, QA>(g, st, what);
        default: return launch_gemm_act<MODE, DQRM_ACT_NONE, QA>(g, st, what);
    }
}

}  // namespace

int dqrm_internal::check_act(int act, const char* what) {
    if (act < DQRM_ACT_NONE || act > DQRM_ACT_SIGMOID)
        return set_error(DQRM_E_INVALID, "%s: act must be DQRM_ACT_NONE, _RELU or _SIGMOID (got %d)", what, act);
    return DQRM_OK;
}

int dqrm_internal::check_linear(const dqrm_linear* l, int quantized, const char* what) {
    if (!l) return set_error(DQRM_E_INVALID, "%s: null layer", what);
    if (l->in_features < 1 || l->out_features < 1)
        return set_error(DQRM_E_INVALID, "%s: in_features / out_features must be positive (got %d / %d)", what,
                         l->in_features, l->out_features);
    if (!l->weight || !l->bias) return set_error(DQRM_E_INVALID, "%s: null weight / bias", what);
    if (quantized) {
        if (l->weight_bit < 2 || l->weight_bit > 32 || l->bias_bit < 2 || l->bias_bit > 32)
            return set_error(DQRM_E_INVALID, "%s: weight_bit / bias_bit must be 2..32 (got %d / %d)", what,
                             l->weight_bit, l->bias_bit);
        if (!l->weight_integer || !l->bias_integer || !l->scale)
            return set_error(DQRM_E_INVALID, "%s: null weight_integer / bias_integer / scale", what);
    }
    return DQRM_OK;
}

namespace {

using dqrm_internal::check_act;
using dqrm_internal::check_linear;

// the integer-activation calls: one-float prev and the [O] / [1] out_scale
int check_qact(const float* prev, const float* out_scale, const char* what) {
    if (!prev || !out_scale) return set_error(DQRM_E_INVALID, "%s: null prev / out_scale", what);
    return DQRM_OK;
}

// dqrm_linear_wquant (QA = false: prev and out_scale unused) and dqrm_linear_wquant_qact
template <bool QA>
int linear_wquant(const dqrm_linear* l, const float* prev, float* out_scale, void* stream, const char* what) {
    int rc = check_linear(l, 1, what);
    if (rc) return rc;
    if (QA && (rc = check_qact(prev, out_scale, what))) return rc;
    const int64_t nw = ((int64_t)1 << (l->weight_bit - 1)) - 1, nb = ((int64_t)1 << (l->bias_bit - 1)) - 1;
    QuantArgs a{l->out_features, l->in_features, l->weight, l->bias, l->weight_integer, l->bias_integer,
                l->scale,        (float)nw,      (float)(-nw - 1), (float)nw, (float)(-nb - 1), (float)nb,
                prev,            out_scale};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((l->out_features + QRPW - 1) / QRPW));
    if (l->per_channel) {
        hipLaunchKernelGGL(k_wquant_rows<QA>, grid, dim3(QWG), 0, st, a);
    } else {
        hipLaunchKernelGGL(k_wquant_absmax, dim3(1), dim3(AWG), 0, st, a);
        DQRM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_wquant_tensor<QA>, grid, dim3(QWG), 0, st, a);
    }
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

// dqrm_linear_fwd / _fwd_act / _fwd_qact and dqrm_linear_bwd / _bwd_act / _bwd_qact (`what` names
// the export in errors). QA: quantized, prev and out_scale given.
template <bool QA>
int linear_fwd(const dqrm_linear* l, int quantized, int act, const float* x, const float* prev,
               const float* out_scale, int64_t B, float* y, void* stream, const char* what) {
    int rc = check_linear(l, quantized, what);
    if (rc) return rc;
    if ((rc = check_act(act, what))) return rc;
    if (QA && (rc = check_qact(prev, out_scale, what))) return rc;
    if (B < 0 || B > INT32_MAX) return set_error(DQRM_E_INVALID, "%s: bad batch size", what);
    if (B == 0) return DQRM_OK;
    if (!x || !y) return set_error(DQRM_E_INVALID, "%s: null x / y", what);
    GemmArgs g{};
    g.M = (int)B;
    g.N = l->out_features;
    g.K = l->in_features;
    g.A = x;
    g.B = quantized ? l->weight_integer : l->weight;
    g.C = y;
    g.s = QA ? out_scale : (quantized ? l->scale : nullptr);
    g.s_stride = l->per_channel ? 1 : 0;
    g.bias = quantized ? l->bias_integer : l->bias;
    g.prev = prev;
    return launch_gemm<FWD, QA>(g, act, (hipStream_t)stream, what);
}

template <bool QA>
int linear_bwd(const dqrm_linear* l, int quantized, int act, const float* x, const float* y, const float* dy,
               const float* prev, const float* out_scale, int64_t B, float* dx, float* dw, float* db, void* stream,
               const char* what) {
    int rc = check_linear(l, quantized, what);
    if (rc) return rc;
    if ((rc = check_act(act, what))) return rc;
    if (QA && (rc = check_qact(prev, out_scale, what))) return rc;
    if (B < 1 || B > INT32_MAX) return set_error(DQRM_E_INVALID, "%s: bad batch size", what);
    if (!x || !dy || !dw || !db) return set_error(DQRM_E_INVALID, "%s: null x / dy / dw / db", what);
    if (act != DQRM_ACT_NONE && !y)
        return set_error(DQRM_E_INVALID, "%s: an activation's backward needs the forward's output (null y)", what);
    hipStream_t st = (hipStream_t)stream;
    GemmArgs g{};
    g.Y = act != DQRM_ACT_NONE ? y : nullptr;
    g.s = QA ? out_scale : (quantized ? l->scale : nullptr);
    g.s_stride = l->per_channel ? 1 : 0;
    g.prev = prev;
    g.ws = l->scale;
    if (dx) {
        g.M = (int)B;
        g.N = l->in_features;
        g.K = l->out_features;
        g.A = dy;
        g.B = quantized ? l->weight_integer : l->weight;
        g.C = dx;
        if ((rc = launch_gemm<DX, QA>(g, act, st, what))) return rc;
    }
    g.M = l->out_features;
    g.N = l->in_features;
    g.K = (int)B;
    g.A = dy;
    g.B = x;
    g.C = dw;
    g.db = db;
    return launch_gemm<DW, QA>(g, act, st, what);
}

}  // namespace

extern "C" {

int dqrm_linear_wquant(const dqrm_linear* l, void* stream) {
    return linear_wquant<false>(l, nullptr, nullptr, stream, "dqrm_linear_wquant");
}

int dqrm_linear_wquant_qact(const dqrm_linear* l, const float* prev, float* out_scale, void* stream) {
    return linear_wquant<true>(l, prev, out_scale, stream, "dqrm_linear_wquant_qact");
}

int dqrm_linear_fwd(const dqrm_linear* l, int quantized, const float* x, int64_t B, float* y, void* stream) {
    return linear_fwd<false>(l, quantized, DQRM_ACT_NONE, x, nullptr, nullptr, B, y, stream, "dqrm_linear_fwd");
}

int dqrm_linear_bwd(const dqrm_linear* l, int quantized, const float* x, const float* dy, int64_t B, float* dx,
                    float* dw, float* db, void* stream) {
    return linear_bwd<false>(l, quantized, DQRM_ACT_NONE, x, nullptr, dy, nullptr, nullptr, B, dx, dw, db, stream,
                             "dqrm_linear_bwd");
}

int dqrm_linear_fwd_act(const dqrm_linear* l, int quantized, int act, const float* x, int64_t B, float* y,
                        void* stream) {
    return linear_fwd<false>(l, quantized, act, x, nullptr, nullptr, B, y, stream, "dqrm_linear_fwd_act");
}

int dqrm_linear_bwd_act(const dqrm_linear* l, int quantized, int act, const float* x, const float* y,
                        const float* dy, int64_t B, float* dx, float* dw, float* db, void* stream) {
    return linear_bwd<false>(l, quantized, act, x, y, dy, nullptr, nullptr, B, dx, dw, db, stream,
                             "dqrm_linear_bwd_act");
}

int dqrm_linear_fwd_qact(const dqrm_linear* l, int act, const float* x, const float* prev, const float* out_scale,
                         int64_t B, float* y, void* stream) {
    return linear_fwd<true>(l, 1, act, x, prev, out_scale, B, y, stream, "dqrm_linear_fwd_qact");
}

int dqrm_linear_bwd_qact(const dqrm_linear* l, int act, const float* x, const float* y, const float* dy,
                         const float* prev, const float* out_scale, int64_t B, float* dx, float* dw, float* db,
                         void* stream) {
    return linear_bwd<true>(l, 1, act, x, y, dy, prev, out_scale, B, dx, dw, db, stream, "dqrm_linear_bwd_qact");
}

}  // extern "C"
