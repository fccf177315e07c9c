// dqrm_loss.hip — DLRMLoss: the loss_threshold clamp and the BCE / MSE / weighted-BCE mean loss
// with its gradient, gfx950.
//
// Reference (YangZhou08/Deep_Quantized_Recommendation_Model_DQRM @ 2024-10-24):
//   DLRM_Net.forward's clamp     dlrm_s_pytorch_tb_dp_one_parallel_comm.py:837-839, :877-879
//   loss_fn_wrap                 dlrm_s_pytorch_tb_dp_one_parallel_comm.py:193-212
//     bce / mse: torch.nn.BCELoss / MSELoss(reduction="mean");
//     wbce:      (loss_ws[T.long()] * BCELoss(reduction="none")(Z, T)).mean()
//
// Entry points: dqrm_loss_fwd (ONE launch, no memset: the kernel writes loss[0] itself),
// dqrm_loss_bwd (one launch). Nothing is read back to the host.
//
// Per sample i (all f32, every operation rounded on its own; built with -ffp-contract=off):
//   z    = clamp ? min(max(p, lo), hi) : p                        NaN propagating
//   bce  : l = (t - 1) * max(log1pf(-z), -100) - t * max(logf(z), -100)      (torch's BCELoss)
//          d = (z - t) / max((1 - z) * z, 1e-12f)                 (torch's BCELoss backward)
//   mse  : l = (z - t) * (z - t);   d = 2 * (z - t)
//   wbce : bce's l and d, w = weights[(int64)t]; a class outside [0, num_weights) reads no
//          memory and gives w = NaN
//   term = w * l                    (w == 1 for bce / mse: no multiply, the same bits)
//   g    = (w * d) / (float)B, and 0 where the clamp cut (p < lo or p > hi; a NaN p stays NaN)
//
// THE SUM ORDER, a function of B alone (restated in tests/cpu_loss.py):
//   slot s = i mod 256, s = 0..255, starts at +0.0f and adds its terms i = s, s + 256, ...
//   in ascending i with plain f32 adds; the 256 slots are then folded with
//   slot[s] += slot[s + stride] (s < stride) for stride = 128, 64, 32, 16, 8, 4, 2, 1;
//   S = slot[0] and loss = S / (float)B.
// One workgroup of kSlots threads (4 waves) computes it, thread s owning slot s: strides 128
// and 64 go through LDS, strides 32..1 through wave 0's shuffles. The grid, the device and the
// stream do not enter the order. B <= 2^20 (4096 terms per slot).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/dqrm.h"
#include "dqrm_internal.h"
#include "dqrm_device.h"

namespace {

using dqrm_internal::set_error;

constexpr int kSlots = 256;                   // the forward's one workgroup: a thread per slot
constexpr int64_t kMaxB = (int64_t)1 << 20;   // largest batch of the one-workgroup forward
constexpr int kBatch = 8;                     // elements a thread loads before it computes them
constexpr int EWG = 256;                      // backward: threads per workgroup
constexpr int kMaxElemGroups = 1 << 12;       // backward grid cap (kMaxB / EWG: never grid-strides)

// max(v, floor) that keeps a NaN v (fmaxf would return the floor)
__device__ __forceinline__ float floor_at(float v, float floor) { return v < floor ? floor : v; }

// weights[(int64)t] (the truncation of .long()); NaN for a class outside [0, nw) or a NaN t
__device__ __forceinline__ float class_weight(const float* __restrict__ weights, int nw, float t) {
    if (t > -1.0f && t < (float)nw) {  // (int)t is in [0, nw] here: the conversion is defined
        const int c = (int)t;
        if (c < nw) return weights[c];
    }
    return __builtin_nanf("");
}

// One sample: z, term = w * l and g (see the header comment); returns the term.
template <int KIND>
__device__ __forceinline__ float loss_sample(float pi, float ti, float fB, int clamp, float lo, float hi,
                                             const float* __restrict__ weights, int nw, float& z, float& gi) {
    z = pi;
    if (clamp) {
        z = z < lo ? lo : z;
        z = z > hi ? hi : z;
    }
    float term, d;
    if (KIND == DQRM_LOSS_MSE) {
        const float e = z - ti;
        term = e * e;
        d = 2.0f * e;
    } else {
        const float a = floor_at(log1pf(-z), -100.0f);
        const float b = floor_at(logf(z), -100.0f);
        term = (ti - 1.0f) * a - ti * b;
        d = (z - ti) / floor_at((1.0f - z) * z, 1e-12f);
        if (KIND == DQRM_LOSS_WBCE) {
            const float w = class_weight(weights, nw, ti);
            term = w * term;
            d = w * d;
        }
    }
    gi = (clamp && (pi < lo || pi > hi)) ? 0.0f : d / fB;
    return term;
}

// Thread s owns slot s. Its elements are taken kBatch at a time: the loads of a batch are issued
// together (one memory latency per batch, not per element), the adds stay in ascending i.
template <int KIND>
__global__ void __launch_bounds__(kSlots) k_loss_fwd(const float* __restrict__ p, const float* __restrict__ t,
                                                    int B, int clamp, float lo, float hi,
                                                    const float* __restrict__ weights, int nw,
                                                    float* __restrict__ loss, float* __restrict__ g,
                                                    float* __restrict__ zout, float* __restrict__ terms) {
    __shared__ float slot[kSlots];
    const int s = threadIdx.x;
    const float fB = (float)B;
    float acc = 0.0f;
    for (int base = s; base < B; base += kSlots * kBatch) {
        float pv[kBatch], tv[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const int i = base + k * kSlots;
            pv[k] = i < B ? p[i] : 0.0f;
            tv[k] = i < B ? t[i] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            const int i = base + k * kSlots;
            if (i < B) {
                float z, gi;
                const float term = loss_sample<KIND>(pv[k], tv[k], fB, clamp, lo, hi, weights, nw, z, gi);
                if (g) g[i] = gi;
                if (zout) zout[i] = z;
                if (terms) terms[i] = term;
                acc = acc + term;
            }
        }
    }
    // fold: strides 128 and 64 through LDS, 32..1 inside wave 0
    slot[s] = acc;
    __syncthreads();
    if (s < 128) slot[s] = slot[s] + slot[s + 128];
    __syncthreads();
    if (s < WAVE) {
        float v = slot[s] + slot[s + 64];
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) v = v + __shfl_down(v, o, WAVE);  // lanes < o hold the slots
        if (s == 0) loss[0] = v / fB;
    }
}

// dp = go[0] * g
__global__ void __launch_bounds__(EWG) k_loss_bwd(const float* __restrict__ g, const float* __restrict__ go, int B,
                                                 float* __restrict__ dp) {
    const float u = go[0];
    for (int i = blockIdx.x * EWG + threadIdx.x; i < B; i += gridDim.x * EWG) dp[i] = u * g[i];
}

}  // namespace

extern "C" {

int dqrm_loss_fwd(const dqrm_loss* cfg, const float* p, const float* t, int64_t B, float* loss, float* g, float* z,
                  float* terms, void* stream) {
    const char* what = "dqrm_loss_fwd";
    if (!cfg) return set_error(DQRM_E_INVALID, "%s: null dqrm_loss", what);
    if (cfg->kind != DQRM_LOSS_BCE && cfg->kind != DQRM_LOSS_MSE && cfg->kind != DQRM_LOSS_WBCE)
        return set_error(DQRM_E_INVALID, "%s: unknown kind %d (DQRM_LOSS_BCE / _MSE / _WBCE)", what, cfg->kind);
    if (cfg->kind == DQRM_LOSS_WBCE && (!cfg->weights || cfg->num_weights < 1))
        return set_error(DQRM_E_INVALID, "%s: DQRM_LOSS_WBCE needs weights (num_weights >= 1, got %d)", what,
                         cfg->num_weights);
    if (B < 1 || B > kMaxB)
        return set_error(DQRM_E_INVALID, "%s: B must be 1..%lld (got %lld)", what, (long long)kMaxB, (long long)B);
    if (!p || !t || !loss) return set_error(DQRM_E_INVALID, "%s: null p / t / loss", what);
    hipStream_t st = (hipStream_t)stream;
    const int clamp = cfg->clamp ? 1 : 0;
#define LOSS_LAUNCH(KIND)                                                                                       \
    hipLaunchKernelGGL(k_loss_fwd<KIND>, dim3(1), dim3(kSlots), 0, st, p, t, (int)B, clamp, cfg->lo, cfg->hi, \
                       cfg->weights, cfg->num_weights, loss, g, z, terms)
    if (cfg->kind == DQRM_LOSS_MSE)
        LOSS_LAUNCH(DQRM_LOSS_MSE);
    else if (cfg->kind == DQRM_LOSS_WBCE)
        LOSS_LAUNCH(DQRM_LOSS_WBCE);
    else
        LOSS_LAUNCH(DQRM_LOSS_BCE);
#undef LOSS_LAUNCH
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

int dqrm_loss_bwd(const float* g, const float* go, int64_t B, float* dp, void* stream) {
    const char* what = "dqrm_loss_bwd";
    if (B < 1 || B > kMaxB)
        return set_error(DQRM_E_INVALID, "%s: B must be 1..%lld (got %lld)", what, (long long)kMaxB, (long long)B);
    if (!g || !go || !dp) return set_error(DQRM_E_INVALID, "%s: null g / go / dp", what);
    const int64_t groups = (B + EWG - 1) / EWG;
    hipLaunchKernelGGL(k_loss_bwd, dim3((unsigned)(groups > kMaxElemGroups ? kMaxElemGroups : groups)), dim3(EWG), 0,
                       (hipStream_t)stream, g, go, (int)B, dp);
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

}  // extern "C"
