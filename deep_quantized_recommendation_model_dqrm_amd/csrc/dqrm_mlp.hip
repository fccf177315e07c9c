// dqrm_mlp.hip — a whole MLP stack per host call, and the stack's SGD update fused with the
// requantization the next forward needs, gfx950.
//
// dqrm_mlp_fwd / dqrm_mlp_bwd hold no GEMM code: they validate the whole stack and then call the
// per-layer exports of dqrm_linear.hip (dqrm_linear_wquant, dqrm_linear_fwd_act,
// dqrm_linear_bwd_act) in the order a layer-by-layer caller would, so their bits are those calls'
// bits by construction. What they save is the host's work per layer. dqrm_mlp_fwd_qact /
// dqrm_mlp_bwd_qact are the same over the integer-activation exports (dqrm_linear_*_qact), with
// k_mlp_qact_prepare (below) in the place of the per-layer weight quantization while the stack's
// integers are current.
//
// dqrm_mlp_sgd is the update kernel. Reference (YangZhou08/Deep_Quantized_Recommendation_Model_DQRM
// @ 2024-10-24): sgd_quantized_gradients_parallel_comm.py:642-646 (the MLP branch of
// weight_update_parallel_comm) and the quantization half of QuantLinear.forward
// (quantization_supp/quant_modules_not_quantize_grad.py:121-154), i.e. what dqrm_dense_update and
// dqrm_linear_wquant compute, in their order of operations:
//     W[o,k] = W[o,k] + (nlr * dw[o,k]) [* gscale[o]]
//     s[o]   = fmaxf(max_k |W[o,k]|, 1e-8f) / n;  wi = clamp(rintf(1/s * W + 0));  bi likewise
// One wave per weight row, the rows of ALL layers in one grid: a wave finds its (layer, row) from
// the prefix of row counts in the kernel arguments (the layer descriptors travel by value, hence
// DQRM_MLP_MAX_LAYERS). A per-channel row is finished by the wave that updated it. A per-tensor
// layer needs the maximum over all its rows: launch 1 leaves every row's max|W| in the workspace,
// launch 2 has every wave of the layer reduce those row maxima itself (a maximum does not depend
// on the order it is taken in) and write its row's integers. No atomics, no memset, no workgroup
// waits on another. dqrm_mlp_sgd_multi is the same two kernels over the rows of several stacks'
// layers (a model's bottom and top MLP): one descriptor list, one grid, one launch.
//
// Compiled with -ffp-contract=off: `nlr * dw`, `* gscale` and `W + ...` are separately rounded.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <math.h>

#include "../../include/dqrm.h"
#include "dqrm_internal.h"
#include "dqrm_device.h"

namespace {

using dqrm_internal::set_error;

constexpr int SWG = 256;            // threads per workgroup
constexpr int SRPW = SWG / WAVE;    // weight rows per workgroup (one per wave)

enum { UPDATE_ONLY = 0, REQUANT_ROWS = 1, REQUANT_TENSOR = 2 };

struct SgdLayer {
    float* W;             // [out][in], updated in place
    float* b;             // [out]
    const float* dw;
    const float* db;
    const float* gs;      // [out + 1] gradient scales (rows, then the bias), or null
    float* wi;
    float* bi;
    float* scale;
    float n;              // 2^(weight_bit-1) - 1
    float wlo, whi;       // weight clamp
    float blo, bhi;       // bias clamp
    int out, in;
    int row0;             // the layer's first row in the grid
    int mode;             // UPDATE_ONLY / REQUANT_ROWS / REQUANT_TENSOR
};

struct SgdArgs {
    SgdLayer layer[DQRM_MLP_MAX_LAYERS];
    int num_layers;
    int total_rows;
    float nlr;            // -lr
    float* rowmax;        // [total_rows] workspace (REQUANT_TENSOR layers only)
};

// the wave's row and its layer (both wave-uniform, so the descriptor is read with scalar loads)
__device__ __forceinline__ bool locate(const SgdArgs& a, int& row, int& l) {
    row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SRPW + threadIdx.x / WAVE));
    if (row >= a.total_rows) return false;
    l = 0;
    while (l + 1 < a.num_layers && row >= a.layer[l + 1].row0) ++l;
    return true;
}

// Launch 1: the update of one weight row and its bias element; a per-channel row's scale and
// integers; a per-tensor row's max|W| into the workspace.
__global__ void __launch_bounds__(SWG) k_mlp_sgd(SgdArgs a) {
    int row, l;
    if (!locate(a, row, l)) return;
    const SgdLayer& d = a.layer[l];
    const int o = row - d.row0, lane = threadIdx.x % WAVE, in = d.in;
    float* w = d.W + (int64_t)o * in;
    const float* __restrict__ g = d.dw + (int64_t)o * in;
    const float nlr = a.nlr;
    float m = 0.0f, bv = 0.0f;
    if (d.gs != nullptr) {
        const float sc = d.gs[o];
        for (int k = lane; k < in; k += WAVE) {
            const float v = w[k] + (nlr * g[k]) * sc;
            w[k] = v;
            m = fmaxf(m, fabsf(v));
        }
        if (lane == 0) d.b[o] = bv = d.b[o] + (nlr * d.db[o]) * d.gs[d.out];
    } else {
        for (int k = lane; k < in; k += WAVE) {
            const float v = w[k] + nlr * g[k];
            w[k] = v;
            m = fmaxf(m, fabsf(v));
        }
        if (lane == 0) d.b[o] = bv = d.b[o] + nlr * d.db[o];
    }
    if (d.mode == UPDATE_ONLY) return;
    m = wave_max(m);
    if (d.mode == REQUANT_TENSOR) {
        if (lane == 0) a.rowmax[row] = m;
        return;
    }
    const float s = fmaxf(m, 1e-8f) / d.n;
    const float rcp = 1.0f / s;
    float* __restrict__ wi = d.wi + (int64_t)o * in;
    for (int k = lane; k < in; k += WAVE) wi[k] = fake_quant(w[k], rcp, d.wlo, d.whi);  // the lane's own stores
    if (lane == 0) {
        d.scale[o] = s;
        d.bi[o] = fake_quant(bv, rcp, d.blo, d.bhi);
    }
}

// Launch 2 (only when a quantized layer is per tensor): every wave of such a layer takes the
// maximum over the layer's row maxima and writes its row's integers; row 0 also writes scale[0].
__global__ void __launch_bounds__(SWG) k_mlp_requant_tensor(SgdArgs a) {
    int row, l;
    if (!locate(a, row, l)) return;
    const SgdLayer& d = a.layer[l];
    if (d.mode != REQUANT_TENSOR) return;
    const int o = row - d.row0, lane = threadIdx.x % WAVE, in = d.in;
    const float* __restrict__ rm = a.rowmax + d.row0;
    float m = 0.0f;
    for (int r = lane; r < d.out; r += WAVE) m = fmaxf(m, rm[r]);
    m = wave_max(m);
    const float s = fmaxf(m, 1e-8f) / d.n;
    const float rcp = 1.0f / s;
    const float* __restrict__ w = d.W + (int64_t)o * in;
    float* __restrict__ wi = d.wi + (int64_t)o * in;
    for (int k = lane; k < in; k += WAVE) wi[k] = fake_quant(w[k], rcp, d.wlo, d.whi);
    if (lane == 0) {
        d.bi[o] = fake_quant(d.b[o], rcp, d.blo, d.bhi);
        if (o == 0) d.scale[0] = s;
    }
}

// ------------------------------------------------------------------------------ qact prepare
// The activation-scale half of dqrm_linear_wquant_qact for every layer of a stack whose weight
// integers and scales are current (dqrm_linear.hip's quant_bias<true>, q_m_n_q_g.py:150-154):
//     p_0 = prev[0];  p_(l+1) = scale_l[0] * p_l          (layer l's one-element out_scale)
//     c[o] = scale_l[o] * p_l;  out_scale_l[o] = c[o];  bias_integer_l[o] = fake_quant(b_l[o], 1 / c[o])
// Workgroups are dealt to layers by the prefix of their counts in the kernel arguments; a
// workgroup's layer is uniform, so its chain of at most 15 products is scalar loads and scalar
// multiplications, each separately rounded, and the same chain the per-layer calls hand from one
// out_scale to the next. One thread per output. Nothing is read that this launch writes.
constexpr int PWG = 256;            // threads (outputs) per workgroup

struct QactLayer {
    const float* b;       // [out]
    const float* scale;   // [out] per channel, [1] per tensor: current (the caller's promise)
    float* bi;            // [out] bias_integer
    float* cos;           // [out] / [1] out_scale
    float blo, bhi;       // bias clamp
    int out;
    int per_channel;
    int blk0;             // the layer's first workgroup in the grid
};

struct QactArgs {
    QactLayer layer[DQRM_MLP_MAX_LAYERS];
    int num_layers;
    const float* prev;    // [1] the activation scale in front of the stack
};

__global__ void __launch_bounds__(PWG) k_mlp_qact_prepare(QactArgs a) {
    const int blk = blockIdx.x;
    int l = 0;
    while (l + 1 < a.num_layers && blk >= a.layer[l + 1].blk0) ++l;
    float p = a.prev[0];
    for (int j = 0; j < l; ++j) p = a.layer[j].scale[0] * p;
    const QactLayer& d = a.layer[l];
    const int o = (blk - d.blk0) * PWG + (int)threadIdx.x;
    if (o >= d.out) return;
    const float s = d.per_channel ? d.scale[o] : d.scale[0];
    const float c = s * p;
    if (d.per_channel) d.cos[o] = c;
    else if (o == 0) d.cos[0] = c;
    d.bi[o] = fake_quant(d.b[o], 1.0f / c, d.blo, d.bhi);
}

}  // namespace

// ------------------------------------------------------------------------------ validation
// the stack's own fields, and every layer as dqrm_linear.hip checks it ("<what>: layer <i>: <fault>")
int dqrm_internal::check_mlp(const dqrm_mlp* m, const char* what) {
    if (!m) return set_error(DQRM_E_INVALID, "%s: null stack", what);
    if (m->num_layers < 1 || m->num_layers > DQRM_MLP_MAX_LAYERS)
        return set_error(DQRM_E_INVALID, "%s: num_layers must be 1..%d (got %d)", what, DQRM_MLP_MAX_LAYERS,
                         m->num_layers);
    if (!m->layers || !m->quantized || !m->act)
        return set_error(DQRM_E_INVALID, "%s: null layers / quantized / act array", what);
    for (int i = 0; i < m->num_layers; ++i) {
        const dqrm_linear* l = &m->layers[i];
        char who[96];
        snprintf(who, sizeof(who), "%s: layer %d", what, i);
        int rc = check_linear(l, m->quantized[i], who);
        if (rc) return rc;
        if (i > 0 && l->in_features != m->layers[i - 1].out_features)
            return set_error(DQRM_E_INVALID, "%s: in_features %d does not match layer %d's out_features %d", who,
                             l->in_features, i - 1, m->layers[i - 1].out_features);
        if ((rc = check_act(m->act[i], who))) return rc;
    }
    return DQRM_OK;
}

bool dqrm_internal::has_tensor_layer(const dqrm_mlp* m) {
    for (int i = 0; i < m->num_layers; ++i)
        if (m->quantized[i] && !m->layers[i].per_channel) return true;
    return false;
}

// an integer-activation stack: every layer quantized (the reference's scale chain breaks at a
// full-precision layer: its forward returns no scale), only the last one per channel (a [out]
// out_scale cannot be the next layer's one-element prev), the scale in front and one out_scale each
int dqrm_internal::check_mlp_qact(const dqrm_mlp* m, const float* prev, float* const* out_scale, const char* what) {
    int rc = check_mlp(m, what);
    if (rc) return rc;
    for (int i = 0; i < m->num_layers; ++i) {
        if (!m->quantized[i])
            return set_error(DQRM_E_INVALID, "%s: layer %d is full precision: an integer-activation stack's scale "
                                             "chain needs every layer quantized", what, i);
        if (m->layers[i].per_channel && i + 1 < m->num_layers)
            return set_error(DQRM_E_INVALID, "%s: layer %d is per_channel: only the last layer may be (its out_scale "
                                             "is the next layer's one-element prev)", what, i);
    }
    if (!prev) return set_error(DQRM_E_INVALID, "%s: null prev", what);
    if (!out_scale) return set_error(DQRM_E_INVALID, "%s: null out_scale array", what);
    for (int i = 0; i < m->num_layers; ++i)
        if (!out_scale[i]) return set_error(DQRM_E_INVALID, "%s: null out_scale[%d]", what, i);
    return DQRM_OK;
}

namespace {

using dqrm_internal::check_mlp;
using dqrm_internal::check_mlp_qact;
using dqrm_internal::has_tensor_layer;

int check_flags(uint32_t flags, uint32_t known, const char* what) {
    if (flags & ~known) return set_error(DQRM_E_INVALID, "%s: unknown flags 0x%x", what, flags);
    return DQRM_OK;
}

// an array of L device pointers, none null
int check_ptrs(const void* const* p, int L, const char* name, const char* what) {
    if (!p) return set_error(DQRM_E_INVALID, "%s: null %s array", what, name);
    for (int i = 0; i < L; ++i)
        if (!p[i]) return set_error(DQRM_E_INVALID, "%s: null %s[%d]", what, name, i);
    return DQRM_OK;
}

// widest tensor between two layers (0 for a stack of one layer)
int64_t max_hidden(const dqrm_mlp* m) {
    int64_t w = 0;
    for (int i = 0; i + 1 < m->num_layers; ++i) w = m->layers[i].out_features > w ? m->layers[i].out_features : w;
    return w;
}

int64_t total_rows(const dqrm_mlp* m) {
    int64_t r = 0;
    for (int i = 0; i < m->num_layers; ++i) r += m->layers[i].out_features;
    return r;
}

// one layer's descriptor of the update grid; requant: refresh its integers and scale too
void fill_layer(SgdLayer& d, const dqrm_linear* l, bool requant, const float* dw, const float* db, const float* gs,
                int row0) {
    d.W = const_cast<float*>(l->weight);
    d.b = const_cast<float*>(l->bias);
    d.dw = dw;
    d.db = db;
    d.gs = gs;
    d.out = l->out_features;
    d.in = l->in_features;
    d.row0 = row0;
    d.mode = UPDATE_ONLY;
    if (requant) {
        const int64_t nw = ((int64_t)1 << (l->weight_bit - 1)) - 1, nb = ((int64_t)1 << (l->bias_bit - 1)) - 1;
        d.wi = l->weight_integer;
        d.bi = l->bias_integer;
        d.scale = l->scale;
        d.n = (float)nw;
        d.wlo = (float)(-nw - 1);
        d.whi = (float)nw;
        d.blo = (float)(-nb - 1);
        d.bhi = (float)nb;
        d.mode = l->per_channel ? REQUANT_ROWS : REQUANT_TENSOR;
    }
}

// the update's launch, and the per-tensor layers' second one
int launch_sgd(const SgdArgs& a, bool two, hipStream_t st) {
    const dim3 grid((unsigned)((a.total_rows + SRPW - 1) / SRPW));
    hipLaunchKernelGGL(k_mlp_sgd, grid, dim3(SWG), 0, st, a);
    DQRM_HIP_TRY(hipGetLastError());
    if (two) {
        hipLaunchKernelGGL(k_mlp_requant_tensor, grid, dim3(SWG), 0, st, a);
        DQRM_HIP_TRY(hipGetLastError());
    }
    return DQRM_OK;
}

// several stacks for one update launch: each a valid stack, DQRM_MLP_MAX_LAYERS layers in all
int check_stacks(const dqrm_mlp* const* stacks, int num_stacks, const char* what) {
    if (!stacks) return set_error(DQRM_E_INVALID, "%s: null stacks array", what);
    if (num_stacks < 1 || num_stacks > DQRM_MLP_MAX_LAYERS)
        return set_error(DQRM_E_INVALID, "%s: num_stacks must be 1..%d (got %d)", what, DQRM_MLP_MAX_LAYERS, num_stacks);
    int L = 0;
    for (int s = 0; s < num_stacks; ++s) {
        int rc = check_mlp(stacks[s], what);
        if (rc) return rc;
        L += stacks[s]->num_layers;
    }
    if (L > DQRM_MLP_MAX_LAYERS)
        return set_error(DQRM_E_INVALID, "%s: the stacks have %d layers in all, at most %d fit one launch", what, L,
                         DQRM_MLP_MAX_LAYERS);
    return DQRM_OK;
}

// dqrm_mlp_sgd_workspace_bytes (one stack) and dqrm_mlp_sgd_multi_workspace_bytes
size_t sgd_workspace_bytes(const dqrm_mlp* const* stacks, int num_stacks, const char* what) {
    if (check_stacks(stacks, num_stacks, what)) return 0;
    int64_t rows = 0;
    bool tensor = false;
    for (int s = 0; s < num_stacks; ++s) {
        rows += total_rows(stacks[s]);
        tensor = tensor || has_tensor_layer(stacks[s]);
    }
    return tensor ? (size_t)rows * sizeof(float) : 0;
}

// dqrm_mlp_sgd (one stack) and dqrm_mlp_sgd_multi; ws_query: the export's workspace query, for the text
int sgd_stacks(const dqrm_mlp* const* stacks, int num_stacks, uint32_t flags, const float* const* dw,
               const float* const* db, const float* const* gscale, float lr, void* workspace, size_t workspace_bytes,
               void* stream, const char* what, const char* ws_query) {
    int rc = check_stacks(stacks, num_stacks, what);
    if (rc) return rc;
    if ((rc = check_flags(flags, DQRM_MLP_REQUANT, what))) return rc;
    int L = 0;
    int64_t rows = 0;
    bool tensor = false;
    for (int s = 0; s < num_stacks; ++s) {
        L += stacks[s]->num_layers;
        rows += total_rows(stacks[s]);
        tensor = tensor || has_tensor_layer(stacks[s]);
    }
    if ((rc = check_ptrs((const void* const*)dw, L, "dw", what))) return rc;
    if ((rc = check_ptrs((const void* const*)db, L, "db", what))) return rc;
    if (gscale && (rc = check_ptrs((const void* const*)gscale, L, "gscale", what))) return rc;
    if (rows > INT32_MAX) return set_error(DQRM_E_CAPACITY, "%s: %lld weight rows exceed the grid's index range", what,
                                           (long long)rows);
    const bool requant = (flags & DQRM_MLP_REQUANT) != 0;
    const bool two = requant && tensor;
    if (two && (!workspace || workspace_bytes < (size_t)rows * sizeof(float)))
        return set_error(DQRM_E_INVALID, "%s: workspace of %zu bytes, %s asks for %zu", what,
                         workspace ? workspace_bytes : (size_t)0, ws_query, (size_t)rows * sizeof(float));
    // the stacks' layers back to back: one descriptor list, one grid over all their rows
    SgdArgs a{};
    int k = 0, row0 = 0;
    for (int s = 0; s < num_stacks; ++s) {
        const dqrm_mlp* m = stacks[s];
        for (int i = 0; i < m->num_layers; row0 += m->layers[i].out_features, ++i, ++k)
            fill_layer(a.layer[k], &m->layers[i], requant && m->quantized[i], dw[k], db[k],
                       gscale ? gscale[k] : nullptr, row0);
    }
    a.num_layers = L;
    a.total_rows = (int)rows;
    a.nlr = -lr;
    a.rowmax = two ? (float*)workspace : nullptr;
    return launch_sgd(a, two, (hipStream_t)stream);
}

// dqrm_mlp_bwd (prev == out_scale == NULL) and dqrm_mlp_bwd_qact on a stack already checked
int stack_bwd(const dqrm_mlp* m, const float* x, const float* const* y, const float* dy, const float* prev,
              float* const* out_scale, int64_t B, float* dx, float* const* dw, float* const* db, void* scratch,
              size_t scratch_bytes, void* stream, const char* what) {
    int rc;
    if (B < 1 || B > INT32_MAX) return set_error(DQRM_E_INVALID, "%s: bad batch size", what);
    if (!x || !dy) return set_error(DQRM_E_INVALID, "%s: null x / dy", what);
    const int L = m->num_layers;
    if ((rc = check_ptrs((const void* const*)y, L, "y", what))) return rc;
    if ((rc = check_ptrs((const void* const*)dw, L, "dw", what))) return rc;
    if ((rc = check_ptrs((const void* const*)db, L, "db", what))) return rc;
    const size_t half = (size_t)B * (size_t)max_hidden(m) * sizeof(float);
    if (half && (!scratch || scratch_bytes < 2 * half))
        return set_error(DQRM_E_INVALID, "%s: scratch of %zu bytes, dqrm_mlp_bwd_scratch_bytes asks for %zu", what,
                         scratch ? scratch_bytes : (size_t)0, 2 * half);
    float* buf[2] = {(float*)scratch, (float*)((char*)scratch + half)};
    for (int i = L - 1; i >= 0; --i) {
        // layer i's dx is layer i-1's dy: buf[i & 1] is written while buf[(i + 1) & 1] is read
        const float* dyi = i == L - 1 ? dy : buf[(i + 1) & 1];
        float* dxi = i == 0 ? dx : buf[i & 1];
        const float* xi = i ? y[i - 1] : x;
        if (out_scale)
            rc = dqrm_linear_bwd_qact(&m->layers[i], m->act[i], xi, y[i], dyi, i ? out_scale[i - 1] : prev,
                                      out_scale[i], B, dxi, dw[i], db[i], stream);
        else
            rc = dqrm_linear_bwd_act(&m->layers[i], m->quantized[i] != 0, m->act[i], xi, y[i], dyi, B, dxi, dw[i],
                                     db[i], stream);
        if (rc) return rc;
    }
    return DQRM_OK;
}

// the prepare launch for a stack check_mlp_qact passed
int launch_qact_prepare(const dqrm_mlp* m, const float* prev, float* const* out_scale, hipStream_t st) {
    QactArgs a{};
    int blk = 0;
    for (int i = 0; i < m->num_layers; ++i) {
        const dqrm_linear* l = &m->layers[i];
        const int64_t nb = ((int64_t)1 << (l->bias_bit - 1)) - 1;
        QactLayer& d = a.layer[i];
        d.b = l->bias;
        d.scale = l->scale;
        d.bi = l->bias_integer;
        d.cos = out_scale[i];
        d.blo = (float)(-nb - 1);
        d.bhi = (float)nb;
        d.out = l->out_features;
        d.per_channel = l->per_channel != 0;
        d.blk0 = blk;
        blk += (l->out_features + PWG - 1) / PWG;
    }
    a.num_layers = m->num_layers;
    a.prev = prev;
    hipLaunchKernelGGL(k_mlp_qact_prepare, dim3((unsigned)blk), dim3(PWG), 0, st, a);
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

}  // namespace

extern "C" {

int dqrm_mlp_fwd(const dqrm_mlp* m, uint32_t flags, const float* x, int64_t B, float* const* y, void* stream) {
    const char* what = "dqrm_mlp_fwd";
    int rc = check_mlp(m, what);
    if (rc) return rc;
    if ((rc = check_flags(flags, DQRM_MLP_FRESH, what))) return rc;
    if (B < 0 || B > INT32_MAX) return set_error(DQRM_E_INVALID, "%s: bad batch size", what);
    if (!y) return set_error(DQRM_E_INVALID, "%s: null y array", what);
    if (B == 0) return DQRM_OK;
    if (!x) return set_error(DQRM_E_INVALID, "%s: null x", what);
    if ((rc = check_ptrs((const void* const*)y, m->num_layers, "y", what))) return rc;
    for (int i = 0; i < m->num_layers; ++i) {
        const dqrm_linear* l = &m->layers[i];
        if (m->quantized[i] && !(flags & DQRM_MLP_FRESH) && (rc = dqrm_linear_wquant(l, stream))) return rc;
        if ((rc = dqrm_linear_fwd_act(l, m->quantized[i] != 0, m->act[i], i ? y[i - 1] : x, B, y[i], stream)))
            return rc;
    }
    return DQRM_OK;
}

size_t dqrm_mlp_bwd_scratch_bytes(const dqrm_mlp* m, int64_t B) {
    if (check_mlp(m, "dqrm_mlp_bwd_scratch_bytes") || B < 0 || B > INT32_MAX) return 0;
    return (size_t)2 * (size_t)B * (size_t)max_hidden(m) * sizeof(float);
}

int dqrm_mlp_bwd(const dqrm_mlp* m, const float* x, const float* const* y, const float* dy, int64_t B, float* dx,
                 float* const* dw, float* const* db, void* scratch, size_t scratch_bytes, void* stream) {
    const char* what = "dqrm_mlp_bwd";
    int rc = check_mlp(m, what);
    if (rc) return rc;
    return stack_bwd(m, x, y, dy, nullptr, nullptr, B, dx, dw, db, scratch, scratch_bytes, stream, what);
}

int dqrm_mlp_qact_prepare(const dqrm_mlp* m, const float* prev, float* const* out_scale, void* stream) {
    int rc = check_mlp_qact(m, prev, out_scale, "dqrm_mlp_qact_prepare");
    if (rc) return rc;
    return launch_qact_prepare(m, prev, out_scale, (hipStream_t)stream);
}

int dqrm_mlp_fwd_qact(const dqrm_mlp* m, uint32_t flags, const float* x, const float* prev, float* const* out_scale,
                      int64_t B, float* const* y, void* stream) {
    const char* what = "dqrm_mlp_fwd_qact";
    int rc = check_mlp_qact(m, prev, out_scale, what);
    if (rc) return rc;
    if ((rc = check_flags(flags, DQRM_MLP_FRESH, what))) return rc;
    if (B < 0 || B > INT32_MAX) return set_error(DQRM_E_INVALID, "%s: bad batch size", what);
    if (!y) return set_error(DQRM_E_INVALID, "%s: null y array", what);
    if (B > 0) {
        if (!x) return set_error(DQRM_E_INVALID, "%s: null x", what);
        if ((rc = check_ptrs((const void* const*)y, m->num_layers, "y", what))) return rc;
    }
    // B == 0: the out_scales and bias integers are still written, no GEMM is launched
    const bool fresh = (flags & DQRM_MLP_FRESH) != 0;
    if (fresh && (rc = launch_qact_prepare(m, prev, out_scale, (hipStream_t)stream))) return rc;
    for (int i = 0; i < m->num_layers; ++i) {
        const dqrm_linear* l = &m->layers[i];
        const float* p = i ? out_scale[i - 1] : prev;
        if (!fresh && (rc = dqrm_linear_wquant_qact(l, p, out_scale[i], stream))) return rc;
        if (B > 0 && (rc = dqrm_linear_fwd_qact(l, m->act[i], i ? y[i - 1] : x, p, out_scale[i], B, y[i], stream)))
            return rc;
    }
    return DQRM_OK;
}

int dqrm_mlp_bwd_qact(const dqrm_mlp* m, const float* x, const float* const* y, const float* dy, const float* prev,
                      float* const* out_scale, int64_t B, float* dx, float* const* dw, float* const* db,
                      void* scratch, size_t scratch_bytes, void* stream) {
    const char* what = "dqrm_mlp_bwd_qact";
    int rc = check_mlp_qact(m, prev, out_scale, what);
    if (rc) return rc;
    return stack_bwd(m, x, y, dy, prev, out_scale, B, dx, dw, db, scratch, scratch_bytes, stream, what);
}

size_t dqrm_mlp_sgd_workspace_bytes(const dqrm_mlp* m) {
    return sgd_workspace_bytes(&m, 1, "dqrm_mlp_sgd_workspace_bytes");
}

int dqrm_mlp_sgd(const dqrm_mlp* m, uint32_t flags, const float* const* dw, const float* const* db,
                 const float* const* gscale, float lr, void* workspace, size_t workspace_bytes, void* stream) {
    return sgd_stacks(&m, 1, flags, dw, db, gscale, lr, workspace, workspace_bytes, stream, "dqrm_mlp_sgd",
                      "dqrm_mlp_sgd_workspace_bytes");
}

size_t dqrm_mlp_sgd_multi_workspace_bytes(const dqrm_mlp* const* stacks, int num_stacks) {
    return sgd_workspace_bytes(stacks, num_stacks, "dqrm_mlp_sgd_multi_workspace_bytes");
}

int dqrm_mlp_sgd_multi(const dqrm_mlp* const* stacks, int num_stacks, uint32_t flags, const float* const* dw,
                       const float* const* db, const float* const* gscale, float lr, void* workspace,
                       size_t workspace_bytes, void* stream) {
    return sgd_stacks(stacks, num_stacks, flags, dw, db, gscale, lr, workspace, workspace_bytes, stream,
                      "dqrm_mlp_sgd_multi", "dqrm_mlp_sgd_multi_workspace_bytes");
}

}  // extern "C"
