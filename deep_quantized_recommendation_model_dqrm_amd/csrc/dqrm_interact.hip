// dqrm_interact.hip — DLRM "dot" feature interaction, forward and backward, gfx950.
//
// Reference (YangZhou08/Deep_Quantized_Recommendation_Model_DQRM @ 2024-10-24):
//   DLRM_Net.interact_features        dlrm_s_pytorch_comm_grad.py:701-806
//     plain:      cat -> bmm(T, T^T) -> Z[:, li, lj] -> cat            (:705-725)
//     quantized:  the same product on 16-bit fake-quantized features   (:741-792)
//   symmetric_linear_quantization_params   quant_utils.py:196-220
//   linear_quantize                        quant_utils.py:75-101     round(1/s * x + 0)
//   SymmetricQuantFunction                 quant_utils.py:316-363    clamp forward, grad / s backward
//
// The problem is small and bound by memory and latency (F = 27 features of D = 16..64 floats
// per sample), so the shape is the plainest one that reads every input once:
//
//   * one 256-thread workgroup per sample, one pass: the grid is B workgroups, several resident
//     per CU (a sample's LDS is 2..7 KB at the real shapes), which cover each other's load latency;
//   * the sample's F x D tile (row 0 = x, row f = emb[f-1]) is staged in LDS with 16-byte loads
//     and stores, row stride D + 4 words: 16-byte aligned, and rows r and r + 1 start 4 banks
//     apart, so the 16-byte reads of threads on consecutive rows fall on different banks. In
//     quantized mode the tile holds the integers, formed on the way in, so both modes share
//     the chain code;
//   * forward: threads map to pairs (i, j), each runs its own chain over k from two LDS rows;
//   * backward: the tile plus the sample's P pair gradients in LDS; threads map to (i, four
//     consecutive k), k fastest (contiguous in LDS), each runs its four chains over j; the
//     coefficient c(i, j) is an LDS read that is the same address for every thread of a row.
//
// Every sum is  acc = 0; acc = fmaf(a, b, acc)  in ascending index, one rounding per product,
// no atomics and no split reductions: a sample's bits depend on its own operands only (and, in
// quantized mode, on the batch's scale, as in the reference). Compiled with -ffp-contract=off:
// `acc * s2`, `g * s2`, `acc / s` and `dr + dT` are separately rounded operations.
//
// dqrm_interact_scale is a maximum, which does not depend on the order it is taken in:
// s = clamp(m, 1e-8) / n is a non-decreasing function of m, so every workgroup folds its own
// maximum into s and the workgroups combine with an integer atomic max on the bit pattern of
// the (positive) result. A 4-byte memset of the output and one launch.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/dqrm.h"
#include "dqrm_internal.h"
#include "dqrm_device.h"

namespace {

using dqrm_internal::set_error;

constexpr int IWG = 256;             // threads per workgroup (one sample)
constexpr int SWG = 256;             // abs-max: threads per workgroup
constexpr int kScaleMaxGrid = 512;   // abs-max: workgroups at most (grid-stride beyond)
constexpr int kPad = 4;              // LDS row stride = D + kPad words
constexpr int kMaxF = 64;
constexpr int kMaxD = 256;
constexpr size_t kPlainLds = 64 * 1024;  // dynamic LDS a launch may ask for without raising the kernel's limit

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct IArgs {
    int F, D, self, quant, P;
    int64_t B;
    int64_t sb, sf;      // emb strides (elements) of the sample and the feature
    const float* x;      // [B][D]
    const float* emb;    // emb[b * sb + f * sf + k]
    const float* scale;  // [1] (quant)
    float lo, hi;        // clamp of the integers (quant)
    float* r;            // fwd: [B][D + P]
    const float* dr;     // bwd: [B][D + P]
    float* dx;           // bwd: [B][D], nullable
    float* demb;         // bwd: [B][F-1][D], nullable
};

// first pair index of row i in the reference's li / lj order:
// for i in range(F): for j in range(i + (1 if itself else 0))
__device__ __forceinline__ int pair_base(int i, int self) { return self ? i * (i + 1) / 2 : i * (i - 1) / 2; }

__device__ __forceinline__ void pair_of(int p, int self, int& i, int& j) {
    int r = (int)((sqrtf(8.0f * (float)p + 1.0f) + (self ? -1.0f : 1.0f)) * 0.5f);
    while (pair_base(r, self) > p) --r;       // the estimate is exact up to rounding: at most
    while (pair_base(r + 1, self) <= p) ++r;  // one step either way
    i = r;
    j = p - pair_base(r, self);
}

// Stage sample b's F x D tile into LDS (the integers in quantized mode). pass != nullptr: also
// copy row 0 (x, unquantized) there, the forward's passthrough.
__device__ __forceinline__ void stage_tile(const IArgs& a, int64_t b, float* tile, float rcp,
                                           float* __restrict__ pass) {
    const int D4 = a.D >> 2, LD = a.D + kPad, n4 = a.F * D4;
    const float* __restrict__ xr = a.x + b * a.D;
    const float* __restrict__ er = a.emb + b * a.sb;
#pragma unroll 2
    for (int e = threadIdx.x; e < n4; e += IWG) {
        const int f = e / D4, q = e - f * D4;
        const float* src = f == 0 ? xr : er + (int64_t)(f - 1) * a.sf;
        f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * q);
        if (pass != nullptr && f == 0) {  // rows of r are not 16-byte aligned: four stores
            pass[4 * q + 0] = v.x;
            pass[4 * q + 1] = v.y;
            pass[4 * q + 2] = v.z;
            pass[4 * q + 3] = v.w;
        }
        if (a.quant) {
            v.x = fake_quant(v.x, rcp, a.lo, a.hi);
            v.y = fake_quant(v.y, rcp, a.lo, a.hi);
            v.z = fake_quant(v.z, rcp, a.lo, a.hi);
            v.w = fake_quant(v.w, rcp, a.lo, a.hi);
        }
        *reinterpret_cast<f32x4*>(tile + f * LD + 4 * q) = v;
    }
}

extern __shared__ __attribute__((aligned(16))) float smem[];

// ------------------------------------------------------------------------------ forward
// One workgroup per sample; thread -> pair (i, j), its own chain over k from two LDS rows.
__global__ void __launch_bounds__(IWG) k_interact_fwd(IArgs a) {
    const int LD = a.D + kPad, D4 = a.D >> 2;
    float* tile = smem;
    const int64_t b = blockIdx.x;
    float rcp = 1.0f, s2 = 1.0f;
    if (a.quant) {
        const float s = a.scale[0];
        rcp = 1.0f / s;
        s2 = s * s;
    }
    float* __restrict__ row = a.r + b * (int64_t)(a.D + a.P);
    stage_tile(a, b, tile, rcp, row);
    __syncthreads();
    for (int p = threadIdx.x; p < a.P; p += IWG) {
        int i, j;
        pair_of(p, a.self, i, j);
        const f32x4* ti = reinterpret_cast<const f32x4*>(tile + i * LD);
        const f32x4* tj = reinterpret_cast<const f32x4*>(tile + j * LD);
        float acc = 0.0f;
#pragma unroll 4
        for (int q = 0; q < D4; ++q) {
            const f32x4 u = ti[q], v = tj[q];
            acc = fmaf(u.x, v.x, acc);
            acc = fmaf(u.y, v.y, acc);
            acc = fmaf(u.z, v.z, acc);
            acc = fmaf(u.w, v.w, acc);
        }
        if (a.quant) acc = acc * s2;
        row[a.D + p] = acc;
    }
}

// ------------------------------------------------------------------------------ backward
// One workgroup per sample; thread -> (i, four consecutive k): four chains over j that share the
// coefficient c(i, j) (one 4-byte LDS read, the same address for every thread of row i) and one
// 16-byte read of row j. The loop body has no branch, so the reads of several j are in flight
// together; the absent j == i term (no self-interaction) keeps the accumulators as they are.
__global__ void __launch_bounds__(IWG) k_interact_bwd(IArgs a) {
    const int LD = a.D + kPad, D4 = a.D >> 2;
    float* tile = smem;
    float* g = tile + a.F * LD;
    const int64_t b = blockIdx.x;
    float s = 1.0f, rcp = 1.0f, s2 = 1.0f;
    if (a.quant) {
        s = a.scale[0];
        rcp = 1.0f / s;
        s2 = s * s;
    }
    const float* __restrict__ drow = a.dr + b * (int64_t)(a.D + a.P);
    stage_tile(a, b, tile, rcp, nullptr);
    for (int p = threadIdx.x; p < a.P; p += IWG) {
        float gv = drow[a.D + p];
        if (a.quant) gv = gv * s2;
        g[p] = gv;
    }
    __syncthreads();
    // work item w = i * D/4 + q: dT[b, i, 4q .. 4q+3]; row 0 is dx's, rows 1.. are demb's
    const int w0 = a.dx != nullptr ? 0 : D4, w1 = a.demb != nullptr ? a.F * D4 : D4;
    const bool skip_diag = !a.self;
    for (int w = w0 + (int)threadIdx.x; w < w1; w += IWG) {
        const int i = w / D4, q = w - i * D4;
        const int bi = pair_base(i, a.self);
        int bj = 0;  // pair_base(j)
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
        for (int j = 0; j < a.F; ++j) {
            const bool diag = j == i, absent = diag && skip_diag;
            const int p = j < i ? bi + j : bj + i;  // p(i, j) for j < i, p(j, i) otherwise
            float c = g[absent ? 0 : p];             // (absent: any valid address, the value is unused)
            c = diag ? c + c : c;
            const f32x4 t = *reinterpret_cast<const f32x4*>(tile + j * LD + 4 * q);
            acc.x = absent ? acc.x : fmaf(c, t.x, acc.x);
            acc.y = absent ? acc.y : fmaf(c, t.y, acc.y);
            acc.z = absent ? acc.z : fmaf(c, t.z, acc.z);
            acc.w = absent ? acc.w : fmaf(c, t.w, acc.w);
            bj += a.self ? j + 1 : j;
        }
        if (a.quant) {
            acc.x = acc.x / s;
            acc.y = acc.y / s;
            acc.z = acc.z / s;
            acc.w = acc.w / s;
        }
        if (i == 0) {
            acc.x = drow[4 * q + 0] + acc.x;  // rows of dr are not 16-byte aligned: four loads
            acc.y = drow[4 * q + 1] + acc.y;
            acc.z = drow[4 * q + 2] + acc.z;
            acc.w = drow[4 * q + 3] + acc.w;
            *reinterpret_cast<f32x4*>(a.dx + b * a.D + 4 * q) = acc;
        } else {
            *reinterpret_cast<f32x4*>(a.demb + b * (int64_t)(a.F - 1) * a.D + 4 * (w - D4)) = acc;
        }
    }
}

// ------------------------------------------------------------------------------ scale
// total4 = B * F * D / 4 sixteen-byte pieces, piece e = ((b * F + f) * D/4 + q)
__global__ void __launch_bounds__(SWG) k_interact_absmax(IArgs a, float n, uint32_t total4, float* out) {
    __shared__ float part[SWG / WAVE];
    const uint32_t D4 = (uint32_t)a.D >> 2, F = (uint32_t)a.F;
    float m = 0.0f;
#pragma unroll 4
    for (uint32_t e = blockIdx.x * SWG + threadIdx.x; e < total4; e += gridDim.x * SWG) {
        const uint32_t row = e / D4, q = e - row * D4;
        const uint32_t b = row / F, f = row - b * F;
        const float* src = f == 0 ? a.x + (int64_t)b * a.D : a.emb + (int64_t)b * a.sb + (int64_t)(f - 1) * a.sf;
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * q);
        m = fmaxf(fmaxf(m, fabsf(v.x)), fmaxf(fabsf(v.y), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    m = wave_max(m);
    if (threadIdx.x % WAVE == 0) part[threadIdx.x / WAVE] = m;
    __syncthreads();
    if (threadIdx.x < WAVE) {
        m = threadIdx.x < SWG / WAVE ? part[threadIdx.x] : 0.0f;
        m = wave_max(m);
        if (threadIdx.x == 0) {
            // atomics on one address serialise: a workgroup whose value does not exceed what is
            // already there has nothing to add (the word only grows)
            unsigned int* word = reinterpret_cast<unsigned int*>(out);
            const unsigned int bits = __float_as_uint(fmaxf(m, 1e-8f) / n);
            if (bits > __atomic_load_n(word, __ATOMIC_RELAXED)) atomicMax(word, bits);
        }
    }
}

// ------------------------------------------------------------------------------ host
int64_t num_pairs(int F, int self) { return (int64_t)F * (F - 1) / 2 + (self ? F : 0); }

bool misaligned(const void* p) { return ((uintptr_t)p & 15u) != 0; }

int check_interact(const dqrm_interact* c, const char* what) {
    if (!c) return set_error(DQRM_E_INVALID, "%s: null interaction config", what);
    if (c->num_features < 2 || c->num_features > kMaxF)
        return set_error(DQRM_E_INVALID, "%s: num_features must be 2..%d (got %d)", what, kMaxF,
                         c->num_features);
    if (c->dim < 4 || c->dim > kMaxD || c->dim % 4 != 0)
        return set_error(DQRM_E_INVALID, "%s: dim must be a multiple of 4 in 4..%d (got %d)", what, kMaxD,
                         c->dim);
    if (c->quant_bits != 0 && (c->quant_bits < 2 || c->quant_bits > 16))
        return set_error(DQRM_E_INVALID, "%s: quant_bits must be 0 or 2..16 (got %d)", what, c->quant_bits);
    if (c->emb_stride_b < 0 || c->emb_stride_b % 4 != 0)
        return set_error(DQRM_E_INVALID, "%s: emb_stride_b must be a non-negative multiple of 4 (got %lld)",
                         what, (long long)c->emb_stride_b);
    if (c->emb_stride_f < 0 || c->emb_stride_f % 4 != 0)
        return set_error(DQRM_E_INVALID, "%s: emb_stride_f must be a non-negative multiple of 4 (got %lld)",
                         what, (long long)c->emb_stride_f);
    return DQRM_OK;
}

// B: 0 <= B and B * F * D / 4 within 32 bits (the abs-max kernel's piece index)
int check_batch(const dqrm_interact* c, int64_t B, const char* what) {
    if (B < 0) return set_error(DQRM_E_INVALID, "%s: B must be >= 0 (got %lld)", what, (long long)B);
    if (B > (int64_t)INT32_MAX / ((int64_t)c->num_features * (c->dim / 4)))
        return set_error(DQRM_E_CAPACITY, "%s: B * num_features * dim / 4 exceeds 2^31 - 1 (B = %lld)", what,
                         (long long)B);
    return DQRM_OK;
}

int check_scale_arg(const dqrm_interact* c, const float* scale, const char* what) {
    if (c->quant_bits != 0 && !scale)
        return set_error(DQRM_E_INVALID, "%s: quant_bits = %d needs a scale (got NULL)", what, c->quant_bits);
    if (c->quant_bits == 0 && scale)
        return set_error(DQRM_E_INVALID, "%s: scale must be NULL when quant_bits is 0", what);
    if (scale && ((uintptr_t)scale & 3u))
        return set_error(DQRM_E_INVALID, "%s: scale is not 4-byte aligned", what);
    return DQRM_OK;
}

#define ICHECK_PTR(p, name)                                                                   \
    do {                                                                                      \
        if (!(p)) return set_error(DQRM_E_INVALID, "%s: null %s", what, name);           \
        if (misaligned(p)) return set_error(DQRM_E_INVALID, "%s: %s is not 16-byte aligned", what, name); \
    } while (0)

IArgs make_args(const dqrm_interact* c, const float* x, const float* emb, int64_t B, const float* scale) {
    IArgs a{};
    a.F = c->num_features;
    a.D = c->dim;
    a.self = c->self_interaction != 0;
    a.quant = c->quant_bits != 0;
    a.P = (int)num_pairs(a.F, a.self);
    a.B = B;
    a.sb = c->emb_stride_b;
    a.sf = c->emb_stride_f;
    a.x = x;
    a.emb = emb;
    a.scale = scale;
    if (a.quant) {
        const int n = (1 << (c->quant_bits - 1)) - 1;
        a.lo = (float)(-n - 1);
        a.hi = (float)n;
    }
    return a;
}

// one workgroup per sample, the sample's LDS as the launch's dynamic shared memory
template <typename K>
int launch_samples(K kernel, const IArgs& a, size_t lds, hipStream_t st) {
    if (lds > kPlainLds)  // F = 64 with D near 256: the tile is past 64 KiB
        DQRM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)a.B), dim3(IWG), lds, st, a);
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

}  // namespace

extern "C" {

int64_t dqrm_interact_out_features(int32_t num_features, int32_t dim, int32_t self_interaction) {
    dqrm_interact c{};
    c.num_features = num_features;
    c.dim = dim;
    if (check_interact(&c, "dqrm_interact_out_features")) return DQRM_E_INVALID;
    return dim + num_pairs(num_features, self_interaction != 0);
}

int dqrm_interact_scale(const dqrm_interact* cfg, const float* x, const float* emb, int64_t B, float* scale,
                        void* stream) {
    const char* what = "dqrm_interact_scale";
    int rc = check_interact(cfg, what);
    if (rc) return rc;
    if (cfg->quant_bits == 0)
        return set_error(DQRM_E_INVALID, "%s: quant_bits is 0 (the plain interaction has no scale)", what);
    if ((rc = check_batch(cfg, B, what))) return rc;
    if ((rc = check_scale_arg(cfg, scale, what))) return rc;
    if (B == 0) return DQRM_OK;
    ICHECK_PTR(x, "x");
    ICHECK_PTR(emb, "emb");
    const IArgs a = make_args(cfg, x, emb, B, scale);
    const uint32_t total4 = (uint32_t)(B * a.F * (a.D / 4));
    const int64_t want = ((int64_t)total4 + SWG * 4 - 1) / (SWG * 4);
    const unsigned grid = (unsigned)(want < kScaleMaxGrid ? want : kScaleMaxGrid);
    hipStream_t st = (hipStream_t)stream;
    DQRM_HIP_TRY(hipMemsetAsync(scale, 0, sizeof(float), st));  // below every clamp(m, 1e-8) / n
    hipLaunchKernelGGL(k_interact_absmax, dim3(grid), dim3(SWG), 0, st, a, a.hi, total4, scale);
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

int dqrm_interact_fwd(const dqrm_interact* cfg, const float* x, const float* emb, int64_t B, const float* scale,
                      float* r, void* stream) {
    const char* what = "dqrm_interact_fwd";
    int rc = check_interact(cfg, what);
    if (rc) return rc;
    if ((rc = check_batch(cfg, B, what))) return rc;
    if ((rc = check_scale_arg(cfg, scale, what))) return rc;
    if (B == 0) return DQRM_OK;
    ICHECK_PTR(x, "x");
    ICHECK_PTR(emb, "emb");
    ICHECK_PTR(r, "r");
    IArgs a = make_args(cfg, x, emb, B, scale);
    a.r = r;
    const size_t per = (size_t)a.F * (a.D + kPad) * sizeof(float);
    return launch_samples(k_interact_fwd, a, per, (hipStream_t)stream);
}

int dqrm_interact_bwd(const dqrm_interact* cfg, const float* x, const float* emb, const float* dr, int64_t B,
                      const float* scale, float* dx, float* demb, void* stream) {
    const char* what = "dqrm_interact_bwd";
    int rc = check_interact(cfg, what);
    if (rc) return rc;
    if ((rc = check_batch(cfg, B, what))) return rc;
    if ((rc = check_scale_arg(cfg, scale, what))) return rc;
    if (B == 0) return DQRM_OK;
    ICHECK_PTR(x, "x");
    ICHECK_PTR(emb, "emb");
    ICHECK_PTR(dr, "dr");
    if (dx && misaligned(dx)) return set_error(DQRM_E_INVALID, "%s: dx is not 16-byte aligned", what);
    if (demb && misaligned(demb)) return set_error(DQRM_E_INVALID, "%s: demb is not 16-byte aligned", what);
    if (!dx && !demb) return DQRM_OK;  // nothing asked for
    IArgs a = make_args(cfg, x, emb, B, scale);
    a.dr = dr;
    a.dx = dx;
    a.demb = demb;
    const size_t per = ((size_t)a.F * (a.D + kPad) + ((a.P + 3) & ~3)) * sizeof(float);
    return launch_samples(k_interact_bwd, a, per, (hipStream_t)stream);
}

}  // extern "C"
