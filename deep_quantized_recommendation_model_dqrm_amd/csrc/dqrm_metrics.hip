// dqrm_metrics.hip — DLRMMetrics: test accuracy and the exact ROC AUC of the reference's test
// loop, kept on the device, gfx950.
//
// Reference (YangZhou08/Deep_Quantized_Recommendation_Model_DQRM @ 2024-10-24):
//   inference()                  dlrm_s_pytorch_tb_dp_one_parallel_comm.py:1304-1404
//     per batch: synchronize, scores / targets to the host             :1348-1355
//     np.sum(np.round(S_test, 0) == T_test)                            :1358-1360
//     sklearn.metrics.roc_auc_score(targets, scores)                   :1387
//
// Entry points: dqrm_metrics_reset (a 32-byte memset), dqrm_metrics_update (ONE launch per
// batch), dqrm_metrics_finish (kFinishLaunches launches, sized from the host's sample count).
// Nothing is read back to the host and no workgroup waits for another.
//
// The arithmetic is stated in include/dqrm.h and restated in tests/cpu_metrics.py. All of it is
// integer except rintf, the compares and `z + 0.0f`. WHERE a key lands in keys[] depends on the
// order in which waves reach their atomic; every OUTPUT (n_pos, n_neg, n_correct, twice_u, flags,
// and the sorted bytes of the smaller class) is a function of the multiset of samples alone:
// integer sums commute, and a sort of bare keys has one result.
//
// finish = k_prep (zero the digit totals and the sum)
//        + 4 x { k_hist     per tile of kTile keys: the 256-bin histogram of the pass's digit,
//                           hist[digit][tile], and the pass's digit totals (one atomic per bin)
//                k_scan     workgroup d: the keys of digits < d (from the totals) + an
//                           exclusive scan of row d of hist, in place
//                k_scatter  per tile: the stable rank of every key inside the tile (wave w owns
//                           keys [w * kTile / 4, ...) of the tile; a lane's rank among its wave's
//                           equal digits is a ballot match, as in the coalesce kernels), the tile
//                           sorted by digit in LDS, written out as up to 256 contiguous runs }
//        + k_search (lb / ub of every element of the other class, uint64 sums, one atomic per
//          workgroup) + k_result.
// The four passes move keys -> ws -> keys -> ws -> keys: the sorted class ends where it was.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dqrm.h"
#include "dqrm_internal.h"
#include "dqrm_device.h"

namespace {

using dqrm_internal::set_error;

typedef unsigned long long u64;

constexpr int kWG = 256;                       // threads per workgroup of every kernel here
constexpr int kWaves = kWG / WAVE;             // 4
constexpr int kTile = DQRM_METRICS_SORT_TILE;  // keys per workgroup of a sort pass
constexpr int kPerWave = kTile / kWaves;       // a wave's contiguous share of a tile
constexpr int kPerLane = kPerWave / WAVE;      // keys a lane holds (16)
constexpr int kBins = 256;                     // 8-bit digits
constexpr int kPasses = 4;
constexpr int kMaxGroups = 2048;               // grid cap of the streaming kernels (grid-stride beyond)
constexpr int kFinishLaunches = 1 + 3 * kPasses + 2;
static_assert(kBins == kWG, "thread d owns bin d");
static_assert(kPerLane * WAVE * kWaves == kTile, "tile shape");

// the workspace of finish: [tmp keys: seen / 2][hist: 256 x tiles][tot: 4 x 256][sum: u64]
struct WsLayout {
    int64_t max_sort;   // keys the smaller class can have: seen / 2
    int64_t tiles;      // sort grid: ceil(max_sort / kTile), at least 1
    size_t hist, tot, sum, bytes;
};

inline WsLayout ws_layout(int64_t seen) {
    WsLayout l;
    l.max_sort = seen / 2;
    l.tiles = l.max_sort > 0 ? (l.max_sort + kTile - 1) / kTile : 1;
    l.hist = (size_t)align16(4 * (l.max_sort > 0 ? l.max_sort : 1));
    l.tot = l.hist + (size_t)align16(4 * (int64_t)kBins * l.tiles);
    l.sum = l.tot + (size_t)(4 * kBins * kPasses);
    l.bytes = l.sum + 16;
    return l;
}

// What every finish kernel derives from the counters: which class is sorted, where, how many.
struct Plan {
    u64 P, N;
    int64_t cnt;        // keys of the sorted (smaller) class
    int64_t sort_off;   // its first key in keys[]
    int64_t other_off;  // the other class's first key
    int64_t other_cnt;
    bool sort_pos;      // the positives are the sorted class
    bool valid;         // the counters fit capacity and the host's seen
};

DQRM_INLINE Plan make_plan(const uint64_t* __restrict__ counters, int64_t capacity, int64_t max_sort) {
    Plan p;
    p.P = counters[0];
    p.N = counters[1];
    p.sort_pos = p.P <= p.N;
    const u64 mn = p.sort_pos ? p.P : p.N;
    p.valid = p.P <= (u64)capacity && p.N <= (u64)capacity && p.P + p.N <= (u64)capacity && mn <= (u64)max_sort;
    p.cnt = p.valid ? (int64_t)mn : 0;
    p.other_cnt = p.valid ? (int64_t)(p.sort_pos ? p.N : p.P) : 0;
    const int64_t neg_off = p.valid ? capacity - (int64_t)p.N : 0;
    p.sort_off = p.sort_pos ? 0 : neg_off;
    p.other_off = p.sort_pos ? neg_off : 0;
    return p;
}

// sum over the workgroup (every thread gets it); red: kWaves words of LDS
DQRM_INLINE uint32_t block_sum(uint32_t v, uint32_t* red) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    __syncthreads();  // red's previous readers are done
    if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += red[w];
    return s;
}

// exclusive scan over the workgroup's kWG values; *total: their sum
DQRM_INLINE uint32_t block_exscan(uint32_t v, uint32_t* red, uint32_t* total) {
    const int lane = threadIdx.x % WAVE, w = threadIdx.x / WAVE;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o, WAVE);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == WAVE - 1) red[w] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        const uint32_t r = red[k];
        if (k < w) before += r;
        all += r;
    }
    *total = all;
    return before + inc - v;
}

// ------------------------------------------------------------------------------------
// update: one launch per batch
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWG) k_metrics_update(const float* __restrict__ z, const float* __restrict__ t,
                                                        int64_t n, uint32_t* __restrict__ keys, int64_t capacity,
                                                        uint64_t* __restrict__ counters) {
    __shared__ uint32_t s_corr[kWaves], s_flag[kWaves];
    const int lane = threadIdx.x % WAVE;
    const u64 below = ((u64)1 << lane) - 1;
    u64* cur = reinterpret_cast<u64*>(counters);
    uint32_t ncorr = 0, flags = 0;
    // the trip count is the same for every lane of the workgroup: the ballots see whole waves
    for (int64_t base = (int64_t)blockIdx.x * kWG; base < n; base += (int64_t)gridDim.x * kWG) {
        const int64_t i = base + threadIdx.x;
        const bool in = i < n;
        const float zi = in ? z[i] : 0.0f, ti = in ? t[i] : 0.0f;
        const float s = zi + 0.0f;  // -0 -> +0
        const uint32_t b = __float_as_uint(s);
        const uint32_t key = (b >> 31) ? ~b : (b | 0x80000000u);
        const bool pos = in && ti == 1.0f, neg = in && ti == 0.0f;
        if (in) {
            if (!pos && !neg) flags |= DQRM_METRICS_F_LABEL;
            if ((b & 0x7F800000u) == 0x7F800000u) flags |= DQRM_METRICS_F_NONFINITE;
            if (rintf(zi) == ti) ncorr += 1;
        }
        const u64 mp = __ballot(pos), mn = __ballot(neg);
        u64 bp = 0, bn = 0;
        if (lane == 0) {  // one returning device-scope add per class and wave
            if (mp) bp = atomicAdd(cur + 0, (u64)__popcll(mp));
            if (mn) bn = atomicAdd(cur + 1, (u64)__popcll(mn));
        }
        bp = __shfl(bp, 0, WAVE);
        bn = __shfl(bn, 0, WAVE);
        if (pos) {
            const u64 at = bp + (u64)__popcll(mp & below);
            if (at < (u64)capacity) keys[at] = key;                 // from the front
        } else if (neg) {
            const u64 at = bn + (u64)__popcll(mn & below);
            if (at < (u64)capacity) keys[capacity - 1 - (int64_t)at] = key;  // from the back
        }
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        ncorr += __shfl_xor(ncorr, o, WAVE);
        flags |= __shfl_xor(flags, o, WAVE);
    }
    if (lane == 0) {
        s_corr[threadIdx.x / WAVE] = ncorr;
        s_flag[threadIdx.x / WAVE] = flags;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // one integer atomic per workgroup (none for a zero)
        uint32_t c = 0, f = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            c += s_corr[w];
            f |= s_flag[w];
        }
        if (c) atomicAdd(cur + 2, (u64)c);
        if (f) atomicOr(cur + 3, (u64)f);
    }
}

// ------------------------------------------------------------------------------------
// finish
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWG) k_metrics_prep(uint32_t* __restrict__ tot, u64* __restrict__ sum) {
    for (int i = threadIdx.x; i < kBins * kPasses; i += kWG) tot[i] = 0u;
    if (threadIdx.x == 0) *sum = 0;
}

DQRM_INLINE int digit_of(uint32_t key, int shift) { return (int)((key >> shift) & 0xFFu); }

// the ping-pong: even passes read keys[] and write the workspace, odd passes the reverse
DQRM_INLINE const uint32_t* pass_src(const Plan& p, int pass, uint32_t* keys, uint32_t* tmp) {
    return (pass & 1) ? tmp : keys + p.sort_off;
}
DQRM_INLINE uint32_t* pass_dst(const Plan& p, int pass, uint32_t* keys, uint32_t* tmp) {
    return (pass & 1) ? keys + p.sort_off : tmp;
}

__global__ void __launch_bounds__(kWG) k_metrics_hist(uint32_t* keys, uint32_t* tmp, int64_t capacity,
                                                      const uint64_t* __restrict__ counters, int64_t max_sort,
                                                      int pass, uint32_t* __restrict__ hist,
                                                      uint32_t* __restrict__ tot) {
    __shared__ uint32_t s_hist[kBins];
    const Plan p = make_plan(counters, capacity, max_sort);
    const int64_t tiles = ceil_div(p.cnt, kTile);
    const int64_t tile = blockIdx.x;
    if (tile >= tiles) return;  // surplus workgroup (uniform)
    const uint32_t* __restrict__ src = pass_src(p, pass, keys, tmp);
    const int shift = 8 * pass;
    s_hist[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t t0 = tile * kTile;
    uint32_t k[kTile / kWG];
#pragma unroll
    for (int j = 0; j < kTile / kWG; ++j) {
        const int64_t i = t0 + j * kWG + threadIdx.x;
        k[j] = i < p.cnt ? src[i] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kTile / kWG; ++j)
        if (t0 + j * kWG + threadIdx.x < p.cnt) atomicAdd(&s_hist[digit_of(k[j], shift)], 1u);
    __syncthreads();
    const uint32_t c = s_hist[threadIdx.x];
    hist[(int64_t)threadIdx.x * tiles + tile] = c;
    if (c) atomicAdd(tot + pass * kBins + threadIdx.x, c);
}

// workgroup d: hist[d][0..tiles) becomes the first output position of tile's keys of digit d
__global__ void __launch_bounds__(kWG) k_metrics_scan(int64_t capacity, const uint64_t* __restrict__ counters,
                                                      int64_t max_sort, int pass, uint32_t* __restrict__ hist,
                                                      const uint32_t* __restrict__ tot) {
    __shared__ uint32_t red[kWaves];
    const Plan p = make_plan(counters, capacity, max_sort);
    const int64_t tiles = ceil_div(p.cnt, kTile);
    if (tiles == 0) return;
    const int d = blockIdx.x;
    uint32_t run = block_sum((int)threadIdx.x < d ? tot[pass * kBins + threadIdx.x] : 0u, red);
    uint32_t* __restrict__ row = hist + (int64_t)d * tiles;
    for (int64_t c0 = 0; c0 < tiles; c0 += kWG) {  // uniform trip count
        const int64_t i = c0 + threadIdx.x;
        const uint32_t v = i < tiles ? row[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exscan(v, red, &total);
        if (i < tiles) row[i] = run + ex;
        run += total;
    }
}

__global__ void __launch_bounds__(kWG) k_metrics_scatter(uint32_t* keys, uint32_t* tmp, int64_t capacity,
                                                         const uint64_t* __restrict__ counters, int64_t max_sort,
                                                         int pass, const uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_off[kWaves][kBins];  // wave w's count of a digit, then its next in-tile position
    __shared__ uint32_t s_gbase[kBins];        // digit d's first output position minus its first in-tile one
    __shared__ uint32_t s_keys[kTile];         // the tile, sorted by digit
    __shared__ uint32_t red[kWaves];
    const Plan p = make_plan(counters, capacity, max_sort);
    const int64_t tiles = ceil_div(p.cnt, kTile);
    const int64_t tile = blockIdx.x;
    if (tile >= tiles) return;  // surplus workgroup (uniform)
    const uint32_t* __restrict__ src = pass_src(p, pass, keys, tmp);
    uint32_t* __restrict__ dst = pass_dst(p, pass, keys, tmp);
    const int shift = 8 * pass;
    const int lane = threadIdx.x % WAVE, w = threadIdx.x / WAVE;
    const u64 below = ((u64)1 << lane) - 1;
    const int64_t t0 = tile * kTile;
    const int64_t left = p.cnt - t0;
    const int tcnt = left < kTile ? (int)left : kTile;  // keys of this tile: a prefix of its slots

#pragma unroll
    for (int q = 0; q < kWaves; ++q) s_off[q][threadIdx.x] = 0u;
    __syncthreads();
    // in-tile slot of key j of this lane: w * kPerWave + j * WAVE + lane (ascending = input order)
    uint32_t k[kPerLane];
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const int sl = w * kPerWave + j * WAVE + lane;
        k[j] = sl < tcnt ? src[t0 + sl] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kPerLane; ++j)
        if (w * kPerWave + j * WAVE + lane < tcnt) atomicAdd(&s_off[w][digit_of(k[j], shift)], 1u);
    __syncthreads();
    {  // thread d: the tile's count of digit d, its exclusive scan, each wave's first position
        const int d = threadIdx.x;
        uint32_t c[kWaves], all = 0;
#pragma unroll
        for (int q = 0; q < kWaves; ++q) {
            c[q] = s_off[q][d];
            all += c[q];
        }
        uint32_t total;
        uint32_t at = block_exscan(all, red, &total);
        s_gbase[d] = hist[(int64_t)d * tiles + tile] - at;  // mod 2^32: + the in-tile position below
#pragma unroll
        for (int q = 0; q < kWaves; ++q) {
            s_off[q][d] = at;
            at += c[q];
        }
    }
    __syncthreads();
    // the wave walks its keys in input order; s_off[w] is private to the wave, whose LDS
    // operations complete in program order
    volatile uint32_t* off = s_off[w];
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const bool in = w * kPerWave + j * WAVE + lane < tcnt;
        const int d = digit_of(k[j], shift);
        u64 peers = __ballot(in);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const u64 m = __ballot(in && bit);
            peers &= bit ? m : ~m;
        }
        if (in) {
            const uint32_t at = off[d];
            const int rank = __popcll(peers & below);
            s_keys[at + rank] = k[j];
            if (rank == 0) off[d] = at + (uint32_t)__popcll(peers);  // the lowest lane of the digit's peers
        }
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    for (int i = threadIdx.x; i < tcnt; i += kWG) {
        const uint32_t key = s_keys[i];
        const uint32_t at = s_gbase[digit_of(key, shift)] + (uint32_t)i;
        if ((int64_t)at < p.cnt) dst[at] = key;  // always true for a consistent scan
    }
}

DQRM_INLINE int64_t lower_bound(const uint32_t* __restrict__ a, int64_t n, uint32_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
DQRM_INLINE int64_t upper_bound(const uint32_t* __restrict__ a, int64_t n, uint32_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kWG) k_metrics_search(const uint32_t* __restrict__ keys, int64_t capacity,
                                                        const uint64_t* __restrict__ counters, int64_t max_sort,
                                                        u64* __restrict__ sum) {
    __shared__ u64 s_sum[kWaves];
    const Plan p = make_plan(counters, capacity, max_sort);
    if (p.cnt == 0 || (int64_t)blockIdx.x * kWG >= p.other_cnt) return;  // surplus workgroup (uniform)
    const uint32_t* __restrict__ sorted = keys + p.sort_off;
    const uint32_t* __restrict__ other = keys + p.other_off;
    u64 acc = 0;
    for (int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x; i < p.other_cnt; i += (int64_t)gridDim.x * kWG) {
        const uint32_t key = other[i];
        const u64 both = (u64)lower_bound(sorted, p.cnt, key) + (u64)upper_bound(sorted, p.cnt, key);
        acc += p.sort_pos ? 2 * p.P - both : both;
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, WAVE);
    if (threadIdx.x % WAVE == 0) s_sum[threadIdx.x / WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += s_sum[w];
        if (s) atomicAdd(sum, s);
    }
}

__global__ void k_metrics_result(int64_t capacity, const uint64_t* __restrict__ counters, int64_t max_sort,
                                 const u64* __restrict__ sum, dqrm_metrics_result* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const Plan p = make_plan(counters, capacity, max_sort);
    out->n_pos = p.P;
    out->n_neg = p.N;
    out->n_correct = counters[2];
    out->twice_u = p.valid ? *sum : 0;
    out->flags = counters[3] | (p.valid ? 0u : DQRM_METRICS_F_COUNT);
}

int check_metrics(const dqrm_metrics* m, const char* what) {
    if (!m) return set_error(DQRM_E_INVALID, "%s: null dqrm_metrics", what);
    if (m->capacity < 1 || m->capacity > DQRM_METRICS_MAX_SAMPLES)
        return set_error(DQRM_E_INVALID, "%s: capacity must be 1..%lld (got %lld)", what,
                         (long long)DQRM_METRICS_MAX_SAMPLES, (long long)m->capacity);
    if (!m->keys || !m->counters) return set_error(DQRM_E_INVALID, "%s: null keys / counters", what);
    return DQRM_OK;
}

}  // namespace

extern "C" {

int dqrm_metrics_reset(const dqrm_metrics* m, void* stream) {
    if (int rc = check_metrics(m, "dqrm_metrics_reset")) return rc;
    DQRM_HIP_TRY(hipMemsetAsync(m->counters, 0, 4 * sizeof(uint64_t), (hipStream_t)stream));
    return DQRM_OK;
}

int dqrm_metrics_update(const dqrm_metrics* m, const float* z, const float* t, int64_t n, int64_t seen_before,
                        void* stream) {
    const char* what = "dqrm_metrics_update";
    if (int rc = check_metrics(m, what)) return rc;
    if (!z || !t) return set_error(DQRM_E_INVALID, "%s: null z / t", what);
    if (n < 1) return set_error(DQRM_E_INVALID, "%s: n must be at least 1 (got %lld)", what, (long long)n);
    if (seen_before < 0 || seen_before > m->capacity || n > m->capacity - seen_before)
        return set_error(DQRM_E_INVALID, "%s: seen_before + n = %lld + %lld exceeds capacity %lld", what,
                         (long long)seen_before, (long long)n, (long long)m->capacity);
    const int64_t groups = (n + kWG - 1) / kWG;
    hipLaunchKernelGGL(k_metrics_update, dim3((unsigned)(groups > kMaxGroups ? kMaxGroups : groups)), dim3(kWG), 0,
                       (hipStream_t)stream, z, t, n, m->keys, m->capacity, m->counters);
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

size_t dqrm_metrics_workspace_bytes(int64_t seen) {
    if (seen < 1 || seen > DQRM_METRICS_MAX_SAMPLES) {
        set_error(DQRM_E_INVALID, "dqrm_metrics_workspace_bytes: seen must be 1..%lld (got %lld)",
                  (long long)DQRM_METRICS_MAX_SAMPLES, (long long)seen);
        return 0;
    }
    return ws_layout(seen).bytes;
}

int dqrm_metrics_finish_launches(int64_t seen) {
    if (seen < 1 || seen > DQRM_METRICS_MAX_SAMPLES)
        return set_error(DQRM_E_INVALID, "dqrm_metrics_finish_launches: seen must be 1..%lld (got %lld)",
                         (long long)DQRM_METRICS_MAX_SAMPLES, (long long)seen);
    return kFinishLaunches;
}

int dqrm_metrics_finish(const dqrm_metrics* m, int64_t seen, dqrm_metrics_result* out_dev, void* ws, size_t ws_bytes,
                        void* stream) {
    const char* what = "dqrm_metrics_finish";
    if (int rc = check_metrics(m, what)) return rc;
    if (seen < 1 || seen > m->capacity)
        return set_error(DQRM_E_INVALID, "%s: seen must be 1..capacity = %lld (got %lld)", what,
                         (long long)m->capacity, (long long)seen);
    if (!out_dev) return set_error(DQRM_E_INVALID, "%s: null out_dev", what);
    const WsLayout l = ws_layout(seen);
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15u) || ws_bytes < l.bytes)
        return set_error(DQRM_E_WORKSPACE, "%s: workspace null, not 16-byte aligned or short (%zu bytes, needs %zu)",
                         what, ws_bytes, l.bytes);
    hipStream_t st = (hipStream_t)stream;
    unsigned char* base = static_cast<unsigned char*>(ws);
    uint32_t* tmp = reinterpret_cast<uint32_t*>(base);
    uint32_t* hist = reinterpret_cast<uint32_t*>(base + l.hist);
    uint32_t* tot = reinterpret_cast<uint32_t*>(base + l.tot);
    u64* sum = reinterpret_cast<u64*>(base + l.sum);
    const int64_t cap = m->capacity;
    const dim3 wg(kWG), tiles((unsigned)l.tiles);
    hipLaunchKernelGGL(k_metrics_prep, dim3(1), wg, 0, st, tot, sum);
    for (int pass = 0; pass < kPasses; ++pass) {
        hipLaunchKernelGGL(k_metrics_hist, tiles, wg, 0, st, m->keys, tmp, cap, m->counters, l.max_sort, pass, hist,
                           tot);
        hipLaunchKernelGGL(k_metrics_scan, dim3(kBins), wg, 0, st, cap, m->counters, l.max_sort, pass, hist, tot);
        hipLaunchKernelGGL(k_metrics_scatter, tiles, wg, 0, st, m->keys, tmp, cap, m->counters, l.max_sort, pass,
                           hist);
    }
    const int64_t groups = (seen + kWG - 1) / kWG;
    hipLaunchKernelGGL(k_metrics_search, dim3((unsigned)(groups > kMaxGroups ? kMaxGroups : groups)), wg, 0, st,
                       m->keys, cap, m->counters, l.max_sort, sum);
    hipLaunchKernelGGL(k_metrics_result, dim3(1), dim3(WAVE), 0, st, cap, m->counters, l.max_sort, sum, out_dev);
    DQRM_HIP_TRY(hipGetLastError());
    return DQRM_OK;
}

}  // extern "C"
