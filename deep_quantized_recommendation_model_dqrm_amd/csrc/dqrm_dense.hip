// dqrm_dense.hip — dense (MLP) layer gradient path of DQRM's data-parallel step, gfx950.
//
// Reference (YangZhou08/Deep_Quantized_Recommendation_Model_DQRM @ 2024-10-24,
// sgd_quantized_gradients_parallel_comm.py):
//   quantize_linear_grad  :892-929  per-channel (weight row) abs-max scale, all_reduce/N,
//                                   SymmetricQuantFunction, all_reduce/N
//   quantize_bias_grad    :931-961  the same with one scale per bias vector
//   grad_update_parallel_comm   MLP branch :337-409  grad.zero_(); grad.add_(buffer)
//   weight_update_parallel_comm MLP branch :630-668  W += (-lr * grad) * s
// and of the simulated-DP buffer (sgd_quantized_gradients.py, one device playing N ranks):
//   grad_buffer_update_added_quantization MLP branch :96-139   error-compensated INT8 accumulate
//   weights_update_added_quantization     MLP branch :381-404  W += -lr * (buffer * (s / N))
//
// Design: every weight row and every bias vector of all bot_l/top_l layers is one
// "channel"; the four phases are ONE launch each for all layers (multi-tensor style: the
// channel table holds the raw grad/param pointers, nothing is copied into a bucket except
// the wire). One wavefront per channel (rows are 13..512 floats in DLRM MLPs), lanes
// striding the row so every load/store instruction of a wave covers 256 contiguous bytes.
// Elementwise and tiny (Kaggle MLP: 0.47 M params): launch/latency-bound, HBM otherwise.
//
// The quantized all-reduce itself is RCCL's (torch.distributed, "nccl" on ROCm): the wire
// holds integer-valued fp16 (exact: |q| <= 128, N <= 16 ranks -> every partial sum is an
// integer of magnitude <= 2048, representable in fp16), so the sum is exact in any
// reduction order and the wire is half the FP32 gradient. int32 otherwise.
// Compiled with -ffp-contract=off: the reference's `1/s*g + 0`, `(-lr*g)*s`, `W + u` are
// separately rounded operations.

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <math.h>

#include "../../include/dqrm.h"
#include "dqrm_internal.h"
#include "dqrm_device.h"

namespace {

using dqrm_internal::set_error;

constexpr int DWG = 256;                 // threads per workgroup
constexpr int CPW = DWG / WAVE;          // channels per workgroup (one per wave)

struct DenseArgs {
    int C;
    float* const* grad;
    float* const* param;
    const int32_t* len;
    const int64_t* wire_off;
};

template <int WT> struct Wire;
template <> struct Wire<DQRM_WIRE_F16> {
    using T = __half;
    static __device__ __forceinline__ T enc(float q) { return __float2half_rn(q); }
    static __device__ __forceinline__ float dec(T v) { return __half2float(v); }
};
template <> struct Wire<DQRM_WIRE_I32> {
    using T = int32_t;
    static __device__ __forceinline__ T enc(float q) { return (int32_t)q; }
    static __device__ __forceinline__ float dec(T v) { return (float)v; }
};
template <> struct Wire<DQRM_WIRE_F32> {
    using T = float;
    static __device__ __forceinline__ T enc(float q) { return q; }
    static __device__ __forceinline__ float dec(T v) { return v; }
};

// s_loc[c] = clamp(max_j |g_j|, 1e-8) / qmax   (max(|min|, |max|) == max |g| for finite g)
__global__ void __launch_bounds__(DWG) k_dense_scale(DenseArgs a, float qmax, float* __restrict__ s_loc) {
    const int c = blockIdx.x * CPW + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (c >= a.C) return;
    const float* __restrict__ g = a.grad[c];
    const int n = a.len[c];
    float m0 = 0.0f, m1 = 0.0f;
    int j = lane;
    for (; j + WAVE < n; j += 2 * WAVE) {  // two loads in flight per lane
        m0 = fmaxf(m0, fabsf(g[j]));
        m1 = fmaxf(m1, fabsf(g[j + WAVE]));
    }
    if (j < n) m0 = fmaxf(m0, fabsf(g[j]));
    const float m = wave_max(fmaxf(m0, m1));
    if (lane == 0) s_loc[c] = fmaxf(m, 1e-8f) / qmax;
}

// scale average in descending rank order (Gloo's one-element all_reduce; every rank
// computes the same bits), then quantize the channel into the wire
template <int WT>
__global__ void __launch_bounds__(DWG) k_dense_quant(DenseArgs a, const float* __restrict__ s_all, int N,
                                                      float inv_n, float lo, float hi, float* __restrict__ s_avg,
                                                      typename Wire<WT>::T* __restrict__ wire) {
    const int c = blockIdx.x * CPW + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (c >= a.C) return;
    const float* __restrict__ g = a.grad[c];
    const int n = a.len[c];
    typename Wire<WT>::T* __restrict__ w = wire + a.wire_off[c];
    if (WT == DQRM_WIRE_F32) {
        for (int j = lane; j < n; j += WAVE) w[j] = Wire<WT>::enc(g[j]);
        return;
    }
    float s = s_all[(int64_t)(N - 1) * a.C + c];
    for (int r = N - 2; r >= 0; --r) s = s + s_all[(int64_t)r * a.C + c];
    s = s * inv_n;
    if (lane == 0) s_avg[c] = s;
    const float rcp = 1.0f / s;
    for (int j = lane; j < n; j += WAVE) w[j] = Wire<WT>::enc(fake_quant(g[j], rcp, lo, hi));
}

// grad = 0 + sum * (1/N)  (quantized) / sum * (1/N)  (FP32)
template <int WT>
__global__ void __launch_bounds__(DWG) k_dense_decode(DenseArgs a, const typename Wire<WT>::T* __restrict__ wire,
                                                       float inv_n) {
    const int c = blockIdx.x * CPW + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (c >= a.C) return;
    float* __restrict__ g = a.grad[c];
    const int n = a.len[c];
    const typename Wire<WT>::T* __restrict__ w = wire + a.wire_off[c];
    if (WT == DQRM_WIRE_F32)  // all_reduce(grad); grad.mul_(1/N)   (:366-369)
        for (int j = lane; j < n; j += WAVE) g[j] = Wire<WT>::dec(w[j]) * inv_n;
    else                      // grad.zero_(); grad.add_(q_sum * (1/N))
        for (int j = lane; j < n; j += WAVE) g[j] = 0.0f + Wire<WT>::dec(w[j]) * inv_n;
}

// param += (-lr * grad) * s   (s == nullptr: param += -lr * grad)
__global__ void __launch_bounds__(DWG) k_dense_update(DenseArgs a, const float* __restrict__ s, float nlr) {
    const int c = blockIdx.x * CPW + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (c >= a.C) return;
    const float* __restrict__ g = a.grad[c];
    float* __restrict__ p = a.param[c];
    const int n = a.len[c];
    if (s != nullptr) {
        const float sc = s[c];
        for (int j = lane; j < n; j += WAVE) p[j] = p[j] + (nlr * g[j]) * sc;
    } else {
        for (int j = lane; j < n; j += WAVE) p[j] = p[j] + nlr * g[j];
    }
}

// One micro-step of the simulated-DP buffer with error compensation
// (sgd_quantized_gradients.py:96-139, quantize_linear_grad / quantize_bias_grad :563-632 with
// err_compensation=True): v = g + e; a channel whose scale is still 0 (the first micro-step
// since zeroing) takes s = clamp(max|v|, 1e-8) / qmax; q = fake_quant(v, 1/s); buf += q;
// e = v - q * s. The quantize pass computes g + e again (the same bits): no row is staged.
__global__ void __launch_bounds__(DWG) k_dense_ec_accumulate(DenseArgs a, float qmax, float lo, float hi,
                                                              float* __restrict__ scale, float* __restrict__ err,
                                                              float* __restrict__ buf) {
    const int c = blockIdx.x * CPW + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (c >= a.C) return;
    const float* __restrict__ g = a.grad[c];
    const int n = a.len[c];
    float* __restrict__ e = err + a.wire_off[c];
    float* __restrict__ b = buf + a.wire_off[c];
    float s = scale[c];  // the same word for the whole wave
    if (s == 0.0f) {
        float m0 = 0.0f, m1 = 0.0f;
        int j = lane;
        for (; j + WAVE < n; j += 2 * WAVE) {  // two loads of each stream in flight per lane
            m0 = fmaxf(m0, fabsf(g[j] + e[j]));
            m1 = fmaxf(m1, fabsf(g[j + WAVE] + e[j + WAVE]));
        }
        if (j < n) m0 = fmaxf(m0, fabsf(g[j] + e[j]));
        s = fmaxf(wave_max(fmaxf(m0, m1)), 1e-8f) / qmax;
        if (lane == 0) scale[c] = s;
    }
    const float rcp = 1.0f / s;
    for (int j = lane; j < n; j += WAVE) {
        const float v = g[j] + e[j];
        const float q = fake_quant(v, rcp, lo, hi);
        b[j] = b[j] + q;
        e[j] = v - q * s;
    }
}

// The buffer's update (sgd_quantized_gradients.py:381-404): param += -lr * (buf * (s / N)),
// s / N a true division.
__global__ void __launch_bounds__(DWG) k_dense_sim_update(DenseArgs a, const float* __restrict__ scale,
                                                           const float* __restrict__ buf, float fn, float nlr) {
    const int c = blockIdx.x * CPW + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (c >= a.C) return;
    float* __restrict__ p = a.param[c];
    const int n = a.len[c];
    const float* __restrict__ b = buf + a.wire_off[c];
    const float t = scale[c] / fn;
    for (int j = lane; j < n; j += WAVE) p[j] = p[j] + nlr * (b[j] * t);
}

int check_dense(const dqrm_dense_set* s) {
    if (!s) return set_error(DQRM_E_INVALID, "dqrm_dense: null dense set");
    if (s->num_channels < 0 || s->total_elems < 0)
        return set_error(DQRM_E_INVALID, "dqrm_dense: negative channel/element count");
    if (s->num_channels > 0 && (!s->grad || !s->param || !s->len || !s->wire_off))
        return set_error(DQRM_E_INVALID, "dqrm_dense: null channel table");
    return DQRM_OK;
}

int check_bits(int bits) {
    if (bits != 32 && (bits < 2 || bits > 16))
        return set_error(DQRM_E_INVALID, "dqrm_dense: bits must be 2..16 or 32 (got %d)", bits);
    return DQRM_OK;
}

DenseArgs args_of(const dqrm_dense_set* s) {
    return DenseArgs{s->num_channels, s->grad, s->param, s->len, s->wire_off};
}

dim3 grid_of(const dqrm_dense_set* s) { return dim3((unsigned)((s->num_channels + CPW - 1) / CPW)); }

}  // namespace

extern "C" {

int dqrm_dense_wire_type(int bits, int num_ranks) {
    if (num_ranks < 1) return DQRM_E_INVALID;
    if (bits == 32) return DQRM_WIRE_F32;
    if (bits < 2 || bits > 16) return DQRM_E_INVALID;
    // |q| <= 2^(bits-1): all partial sums over N ranks exact in fp16 iff N * 2^(bits-1) <= 2048
    if ((int64_t)num_ranks << (bits - 1) <= 2048) return DQRM_WIRE_F16;
    return DQRM_WIRE_I32;
}

int dqrm_dense_grad_scale(const dqrm_dense_set* set, int bits, float* s_loc, void* stream) {
    int rc = check_dense(set);
    if (rc) return rc;
    if ((rc = check_bits(bits))) return rc;
    if (bits == 32) return set_error(DQRM_E_INVALID, "dqrm_dense_grad_scale: no scale for unquantized gradients");
    if (set->num_channels == 0) return DQRM_OK;
    if (!s_loc) return set_error(DQRM_E_INVALID, "dqrm_dense_grad_scale: null s_loc");
    const float qmax = (float)((1 << (bits - 1)) - 1);
    hipLaunchKernelGGL(k_dense_scale, grid_of(set), dim3(DWG), 0, (hipStream_t)stream, args_of(set), qmax, s_loc);
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

int dqrm_dense_grad_quant(const dqrm_dense_set* set, int bits, const float* s_all, int num_ranks, float* s_avg,
                          int wire_type, void* wire, void* stream) {
    int rc = check_dense(set);
    if (rc) return rc;
    if ((rc = check_bits(bits))) return rc;
    if (num_ranks < 1) return set_error(DQRM_E_INVALID, "dqrm_dense_grad_quant: num_ranks < 1");
    if (set->num_channels == 0) return DQRM_OK;
    if (!wire) return set_error(DQRM_E_INVALID, "dqrm_dense_grad_quant: null wire");
    if ((bits == 32) != (wire_type == DQRM_WIRE_F32))
        return set_error(DQRM_E_INVALID, "dqrm_dense_grad_quant: wire type %d does not match bits %d", wire_type, bits);
    if (bits != 32) {
        if (!s_all || !s_avg) return set_error(DQRM_E_INVALID, "dqrm_dense_grad_quant: null scale buffers");
        const int need = dqrm_dense_wire_type(bits, num_ranks);
        if (wire_type == DQRM_WIRE_F16 && need != DQRM_WIRE_F16)
            return set_error(DQRM_E_INVALID, "dqrm_dense_grad_quant: fp16 wire inexact for bits %d, %d ranks",
                             bits, num_ranks);
    }
    const float inv_n = 1.0f / (float)num_ranks;
    const int n = bits == 32 ? 0 : (1 << (bits - 1)) - 1;
    const float lo = (float)(-n - 1), hi = (float)n;
    hipStream_t st = (hipStream_t)stream;
    switch (wire_type) {
        case DQRM_WIRE_F16:
            hipLaunchKernelGGL(k_dense_quant<DQRM_WIRE_F16>, grid_of(set), dim3(DWG), 0, st, args_of(set), s_all,
                               num_ranks, inv_n, lo, hi, s_avg, (__half*)wire);
            break;
        case DQRM_WIRE_I32:
            hipLaunchKernelGGL(k_dense_quant<DQRM_WIRE_I32>, grid_of(set), dim3(DWG), 0, st, args_of(set), s_all,
                               num_ranks, inv_n, lo, hi, s_avg, (int32_t*)wire);
            break;
        case DQRM_WIRE_F32:
            hipLaunchKernelGGL(k_dense_quant<DQRM_WIRE_F32>, grid_of(set), dim3(DWG), 0, st, args_of(set), s_all,
                               num_ranks, inv_n, lo, hi, s_avg, (float*)wire);
            break;
        default:
            return set_error(DQRM_E_INVALID, "dqrm_dense_grad_quant: unknown wire type %d", wire_type);
    }
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

int dqrm_dense_grad_decode(const dqrm_dense_set* set, const void* wire, int wire_type, int num_ranks, void* stream) {
    int rc = check_dense(set);
    if (rc) return rc;
    if (num_ranks < 1) return set_error(DQRM_E_INVALID, "dqrm_dense_grad_decode: num_ranks < 1");
    if (set->num_channels == 0) return DQRM_OK;
    if (!wire) return set_error(DQRM_E_INVALID, "dqrm_dense_grad_decode: null wire");
    const float inv_n = 1.0f / (float)num_ranks;
    hipStream_t st = (hipStream_t)stream;
    switch (wire_type) {
        case DQRM_WIRE_F16:
            hipLaunchKernelGGL(k_dense_decode<DQRM_WIRE_F16>, grid_of(set), dim3(DWG), 0, st, args_of(set),
                               (const __half*)wire, inv_n);
            break;
        case DQRM_WIRE_I32:
            hipLaunchKernelGGL(k_dense_decode<DQRM_WIRE_I32>, grid_of(set), dim3(DWG), 0, st, args_of(set),
                               (const int32_t*)wire, inv_n);
            break;
        case DQRM_WIRE_F32:
            hipLaunchKernelGGL(k_dense_decode<DQRM_WIRE_F32>, grid_of(set), dim3(DWG), 0, st, args_of(set),
                               (const float*)wire, inv_n);
            break;
        default:
            return set_error(DQRM_E_INVALID, "dqrm_dense_grad_decode: unknown wire type %d", wire_type);
    }
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

int dqrm_dense_update(const dqrm_dense_set* set, const float* s, float lr, void* stream) {
    int rc = check_dense(set);
    if (rc) return rc;
    if (set->num_channels == 0) return DQRM_OK;
    hipLaunchKernelGGL(k_dense_update, grid_of(set), dim3(DWG), 0, (hipStream_t)stream, args_of(set), s, -lr);
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

int dqrm_dense_ec_accumulate(const dqrm_dense_set* set, int bits, float* scale, float* err, float* buf,
                             void* stream) {
    int rc = check_dense(set);
    if (rc) return rc;
    if (bits < 2 || bits > 16)
        return set_error(DQRM_E_INVALID, "dqrm_dense_ec_accumulate: bits must be 2..16 (got %d)", bits);
    if (set->num_channels == 0) return DQRM_OK;
    if (!scale || !err || !buf)
        return set_error(DQRM_E_INVALID, "dqrm_dense_ec_accumulate: null scale, err or buf");
    const int n = (1 << (bits - 1)) - 1;
    hipLaunchKernelGGL(k_dense_ec_accumulate, grid_of(set), dim3(DWG), 0, (hipStream_t)stream, args_of(set),
                       (float)n, (float)(-n - 1), (float)n, scale, err, buf);
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

int dqrm_dense_sim_update(const dqrm_dense_set* set, const float* scale, const float* buf, int num_gpus, float lr,
                          void* stream) {
    int rc = check_dense(set);
    if (rc) return rc;
    if (num_gpus < 1) return set_error(DQRM_E_INVALID, "dqrm_dense_sim_update: num_gpus < 1");
    if (set->num_channels == 0) return DQRM_OK;
    if (!scale || !buf) return set_error(DQRM_E_INVALID, "dqrm_dense_sim_update: null scale or buf");
    hipLaunchKernelGGL(k_dense_sim_update, grid_of(set), dim3(DWG), 0, (hipStream_t)stream, args_of(set), scale,
                       buf, (float)num_gpus, -lr);
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

}  // extern "C"
