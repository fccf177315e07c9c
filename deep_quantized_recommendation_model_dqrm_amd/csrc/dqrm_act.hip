// dqrm_act.hip — QuantAct (fake-quantized activations with a running range), gfx950.
//
// Reference (YangZhou08/Deep_Quantized_Recommendation_Model_DQRM @ 2024-10-24,
// quantization_supp/):
//   QuantAct.forward                       quant_modules_not_quantize_grad.py:625-725
//   symmetric_linear_quantization_params   quant_utils.py:196-220
//   linear_quantize                        quant_utils.py:75-101     round(1/s * x + 0)
//   SymmetricQuantFunction                 quant_utils.py:316-363    clamp forward, grad / s backward
//
// Entry points: dqrm_act_quant_workspace_bytes, dqrm_act_quant_fwd, dqrm_act_quant_bwd.
//
// Forward launches (at most three, all on the caller's stream, nothing read back):
//   1. k_act_range_partial  running_stat and numel > kOneGroupMax only: up to kMaxGroups
//                           workgroups, each the min and max of its grid-strided share of x,
//                           written to the workspace (a min / max does not depend on the order
//                           it is taken in, so the grid does not show in the bits);
//   2. k_act_range_update   running_stat only: ONE workgroup reduces the partials (or x itself
//                           when numel <= kOneGroupMax) and its thread 0 applies the reference's
//                           range update to x_min / x_max. The reference branches on the host
//                           (`if self.x_min == self.x_max`, a device-to-host read); here the
//                           branch is taken on the device. Nothing else runs beside this
//                           workgroup on the stream, so no reader sees a half-updated range;
//   3. k_act_quantize       every thread forms scale from x_min / x_max (two uniform loads) and
//                           quantizes its elements; thread 0 of workgroup 0 stores scale[0].
// Without running_stat (a fixed module) only launch 3 runs. Backward: one launch.
//
// Compiled with -ffp-contract=off: `x_min * m + bmin * (1 - m)`, `1/s * x + 0`, `q * s` and
// `(dy * s) / s` are separately rounded operations, as the reference's torch ops are.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/dqrm.h"
#include "dqrm_internal.h"
#include "dqrm_device.h"

namespace {

using dqrm_internal::set_error;

constexpr int RWG = 1024;                   // range kernels: threads per workgroup
constexpr int EWG = 256;                    // elementwise kernels: threads per workgroup
constexpr int64_t kOneGroupMax = 16384;     // up to here the update workgroup reads x itself
constexpr int kMaxGroups = 1024;            // partial workgroups (the workspace holds 2 floats each)
constexpr int64_t kPartialPerGroup = 16384; // elements a partial workgroup takes before the grid is capped
constexpr int kMaxElemGroups = 1 << 16;     // elementwise grid cap (grid-stride beyond)

__device__ __forceinline__ void wave_minmax(float& lo, float& hi) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, WAVE));
        hi = fmaxf(hi, __shfl_xor(hi, o, WAVE));
    }
}

// The workgroup's min / max of the per-thread (lo, hi), valid in thread 0.
__device__ __forceinline__ void group_minmax(float& lo, float& hi) {
    __shared__ float plo[RWG / WAVE], phi[RWG / WAVE];
    wave_minmax(lo, hi);
    if (threadIdx.x % WAVE == 0) {
        plo[threadIdx.x / WAVE] = lo;
        phi[threadIdx.x / WAVE] = hi;
    }
    __syncthreads();
    if (threadIdx.x < WAVE) {
        lo = threadIdx.x < RWG / WAVE ? plo[threadIdx.x] : INFINITY;
        hi = threadIdx.x < RWG / WAVE ? phi[threadIdx.x] : -INFINITY;
        wave_minmax(lo, hi);
    }
}

// launch 1: part[2g] = min, part[2g+1] = max of workgroup g's share (gridDim.x <= numel / RWG,
// so every workgroup has elements)
__global__ void __launch_bounds__(RWG) k_act_range_partial(const float* __restrict__ x, int64_t numel,
                                                          float* __restrict__ part) {
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t e = (int64_t)blockIdx.x * RWG + threadIdx.x; e < numel; e += (int64_t)gridDim.x * RWG) {
        const float v = x[e];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    group_minmax(lo, hi);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = lo;
        part[2 * blockIdx.x + 1] = hi;
    }
}

// launch 2, one workgroup: the batch's range from `groups` partial pairs (groups > 0) or from x,
// then QuantAct.forward:667-678 on x_min[0] / x_max[0]. m1 = (float)(1.0 - (double)momentum), the
// float torch multiplies an f32 tensor with for the Python scalar `1 - momentum`.
__global__ void __launch_bounds__(RWG) k_act_range_update(const float* __restrict__ x, int64_t numel,
                                                         const float* __restrict__ part, int groups, float m,
                                                         float m1, float* __restrict__ x_min,
                                                         float* __restrict__ x_max) {
    float lo = INFINITY, hi = -INFINITY;
    if (groups > 0) {
        for (int g = threadIdx.x; g < groups; g += RWG) {
            lo = fminf(lo, part[2 * g]);
            hi = fmaxf(hi, part[2 * g + 1]);
        }
    } else {
        for (int64_t e = threadIdx.x; e < numel; e += RWG) {
            const float v = x[e];
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
    group_minmax(lo, hi);
    if (threadIdx.x == 0) {
        const float cur_lo = x_min[0], cur_hi = x_max[0];
        float new_lo, new_hi;
        if (cur_lo == cur_hi) {  // "Initialization": an add, as the reference writes it
            new_lo = cur_lo + lo;
            new_hi = cur_hi + hi;
        } else if (m == -1.0f) {
            new_lo = fminf(cur_lo, lo);
            new_hi = fmaxf(cur_hi, hi);
        } else {
            new_lo = cur_lo * m + lo * m1;
            new_hi = cur_hi * m + hi * m1;
        }
        x_min[0] = new_lo;
        x_max[0] = new_hi;
    }
}

DQRM_INLINE float quant_dequant(float v, float rcp, float s, float lo, float hi) {
    return fake_quant(v, rcp, lo, hi) * s;
}

// launch 3: scale = clamp(max(|x_min|, |x_max|), 1e-8) / n; y = clamp(round(1/scale * x + 0)) * scale.
// VEC: x and y are 16-byte aligned, four elements per step and a scalar tail.
template <bool VEC>
__global__ void __launch_bounds__(EWG) k_act_quantize(const float* __restrict__ x, int64_t numel,
                                                     float* __restrict__ y, const float* __restrict__ x_min,
                                                     const float* __restrict__ x_max, float* __restrict__ scale,
                                                     float n, float lo, float hi) {
    const float s = fmaxf(fmaxf(fabsf(x_min[0]), fabsf(x_max[0])), 1e-8f) / n;
    const float rcp = 1.0f / s;
    const int64_t t = (int64_t)blockIdx.x * EWG + threadIdx.x, stride = (int64_t)gridDim.x * EWG;
    if (t == 0) scale[0] = s;
    if (VEC) {
        const int64_t n4 = numel / 4;
        const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
        float4* __restrict__ y4 = reinterpret_cast<float4*>(y);
        for (int64_t e = t; e < n4; e += stride) {
            const float4 v = x4[e];
            y4[e] = make_float4(quant_dequant(v.x, rcp, s, lo, hi), quant_dequant(v.y, rcp, s, lo, hi),
                                quant_dequant(v.z, rcp, s, lo, hi), quant_dequant(v.w, rcp, s, lo, hi));
        }
        for (int64_t e = n4 * 4 + t; e < numel; e += stride) y[e] = quant_dequant(x[e], rcp, s, lo, hi);
    } else {
        for (int64_t e = t; e < numel; e += stride) y[e] = quant_dequant(x[e], rcp, s, lo, hi);
    }
}

// backward: dx = (dy * scale) / scale (the `* correct_output_scale` of :723, then the STE)
__global__ void __launch_bounds__(EWG) k_act_bwd(const float* __restrict__ dy, int64_t numel,
                                                float* __restrict__ dx, const float* __restrict__ scale) {
    const float s = scale[0];
    const int64_t stride = (int64_t)gridDim.x * EWG;
    for (int64_t e = (int64_t)blockIdx.x * EWG + threadIdx.x; e < numel; e += stride) dx[e] = (dy[e] * s) / s;
}

unsigned elem_groups(int64_t work) {
    const int64_t g = (work + EWG - 1) / EWG;
    return (unsigned)(g < 1 ? 1 : (g > kMaxElemGroups ? kMaxElemGroups : g));
}

int partial_groups(int64_t numel) {
    if (numel <= kOneGroupMax) return 0;
    const int64_t g = (numel + kPartialPerGroup - 1) / kPartialPerGroup;
    return (int)(g > kMaxGroups ? kMaxGroups : g);
}

}  // namespace

int dqrm_internal::check_act_quant(const dqrm_act_quant* q, const char* what) {
    if (!q) return set_error(DQRM_E_INVALID, "%s: null dqrm_act_quant", what);
    if (q->activation_bit < 2 || q->activation_bit > 32)
        return set_error(DQRM_E_INVALID, "%s: activation_bit must be 2..32 (got %d)", what, q->activation_bit);
    if (!q->x_min || !q->x_max || !q->scale) return set_error(DQRM_E_INVALID, "%s: null x_min / x_max / scale", what);
    return DQRM_OK;
}

int dqrm_internal::act_quant_fwd_launches(const dqrm_act_quant* q, int64_t numel) {
    if (numel <= 0) return 0;
    return 1 + (q->running_stat ? 1 + (partial_groups(numel) > 0 ? 1 : 0) : 0);
}

extern "C" {

int64_t dqrm_act_quant_workspace_bytes(int64_t numel) {
    if (numel < 0) return set_error(DQRM_E_INVALID, "dqrm_act_quant_workspace_bytes: negative numel");
    return numel > kOneGroupMax ? (int64_t)kMaxGroups * 2 * (int64_t)sizeof(float) : 0;
}

int dqrm_act_quant_fwd(const dqrm_act_quant* q, const float* x, int64_t numel, float* y, void* workspace,
                       void* stream) {
    const char* what = "dqrm_act_quant_fwd";
    int rc = dqrm_internal::check_act_quant(q, what);
    if (rc) return rc;
    if (numel < 0) return set_error(DQRM_E_INVALID, "%s: negative numel", what);
    if (numel == 0) return DQRM_OK;
    if (!x) return set_error(DQRM_E_INVALID, "%s: null x", what);
    if (!y && !q->running_stat)
        return set_error(DQRM_E_INVALID, "%s: null y (a range-only call) needs running_stat", what);
    const int groups = q->running_stat ? partial_groups(numel) : 0;
    if (groups > 0 && !workspace)
        return set_error(DQRM_E_INVALID, "%s: null workspace (dqrm_act_quant_workspace_bytes(%lld) bytes needed)",
                         what, (long long)numel);
    hipStream_t st = (hipStream_t)stream;
    if (q->running_stat) {
        float* part = (float*)workspace;
        if (groups > 0) {
            hipLaunchKernelGGL(k_act_range_partial, dim3((unsigned)groups), dim3(RWG), 0, st, x, numel, part);
            DQRM_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_act_range_update, dim3(1), dim3(RWG), 0, st, x, numel, part, groups, q->momentum,
                           q->one_minus_momentum, q->x_min, q->x_max);
        DQRM_HIP_TRY(hipGetLastError());
    }
    if (y) {
        const int64_t nq = ((int64_t)1 << (q->activation_bit - 1)) - 1;
        const float n = (float)nq, lo = (float)(-nq - 1), hi = (float)nq;
        if ((((uintptr_t)x | (uintptr_t)y) & 15) == 0)
            hipLaunchKernelGGL(k_act_quantize<true>, dim3(elem_groups((numel + 3) / 4)), dim3(EWG), 0, st, x, numel, y,
                               q->x_min, q->x_max, q->scale, n, lo, hi);
        else
            hipLaunchKernelGGL(k_act_quantize<false>, dim3(elem_groups(numel)), dim3(EWG), 0, st, x, numel, y,
                               q->x_min, q->x_max, q->scale, n, lo, hi);
        DQRM_HIP_TRY(hipGetLastError());
    }
    return DQRM_OK;
}

int dqrm_act_quant_bwd(const float* scale, const float* dy, int64_t numel, float* dx, void* stream) {
    const char* what = "dqrm_act_quant_bwd";
    if (!scale) return set_error(DQRM_E_INVALID, "%s: null scale", what);
    if (numel < 0) return set_error(DQRM_E_INVALID, "%s: negative numel", what);
    if (numel == 0) return DQRM_OK;
    if (!dy || !dx) return set_error(DQRM_E_INVALID, "%s: null dy / dx", what);
    hipLaunchKernelGGL(k_act_bwd, dim3(elem_groups(numel)), dim3(EWG), 0, (hipStream_t)stream, dy, numel, dx, scale);
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

}  // extern "C"
