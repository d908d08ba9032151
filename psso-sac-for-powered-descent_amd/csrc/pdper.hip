// pdper.hip -- prioritized replay on the device: the learner's sample and priority update of the
// reference's PrioritizedReplayBuffer (sac_pytorch.py:90-124) as kernels, no host in between.
//
// pd_per_sample draws `batch` distinct items with probability proportional to priority**alpha,
// without replacement -- the distribution of np.random.choice(size, batch, replace=False, p) -- as
// an exponential race: item i gets the key e_i = -log(u_i) / w_i, w_i = priority_i**alpha, u_i its
// own Philox uniform in (0, 1], and the batch smallest keys win, in ascending order (the order of
// numpy's sequential draw).  Positive doubles order as their bit patterns, so the selection is a
// radix select on key bits:
//   k_per_hist    grid-stride over quads of items (one 16-byte priority load, two Philox blocks):
//                 keys, and a histogram of their top 13 bits (sign, exponent, one mantissa bit: bins
//                 a factor sqrt(2) wide), per workgroup in LDS, then one integer atomic per
//                 non-empty bin -- integer counts do not depend on the order of arrival
//   k_per_scan    one workgroup: the bin T that holds the batch-th smallest key
//   k_per_collect the keys again (cheaper than 8 bytes per item stored and re-read); every item in
//                 a bin <= T goes to a candidate list (one atomic counter, bounded capacity)
//   k_per_final   one workgroup: bitonic sort of the candidates by (key, index) in LDS -- which
//                 removes the arrival order of the atomics, so the outputs are reproducible bit for
//                 bit -- then indices, importance weights and the gathered rows
// The expected number of keys below x, sum_i (1 - exp(-w_i x)), is concave in x, so the keys up to
// the top of bin T are at most about sqrt(2) x batch, whatever the priorities; the list holds
// 4 x batch (at least 256).  An overflow drops candidates and raises info[2].
// Importance weights: (size w_j / sum w)^-beta / max over the batch = (w_min / w_j)^beta with w_min
// the smallest selected weight -- the sum over the buffer cancels and is never formed.
#include <hip/hip_runtime.h>

#include "../../include/pdenv.h"
#include "pd_common.h"

namespace {

using namespace pd;

constexpr int kPerBlock = 1024;
constexpr int kPerMaxGrid = 256;          // one workgroup per CU
constexpr int kBinShift = 51;
constexpr int kBins = 4096;               // key bits >> 51 of a non-negative double
constexpr int kCapMax = 4 * PD_PER_MAX_BATCH;
constexpr int kCapMin = 256;
constexpr uint64_t kInfBits = 0x7FF0000000000000ull;
// scratch: histogram, control words, candidate keys, candidate indices
constexpr size_t kOffCtrl = (size_t)kBins * sizeof(uint32_t);
constexpr size_t kOffKeys = kOffCtrl + 64;
enum { kCtrlCount = 0, kCtrlBin = 1, kCtrlExpect = 2, kCtrlFinite = 3 };

int per_capacity(int32_t batch) {
    int c = kCapMin;
    while (c < 4 * (int64_t)batch && c < kCapMax) c <<= 1;
    return c;
}

__device__ __forceinline__ double per_weight(float p, double alpha) { return pow((double)p, alpha); }

// e = -log(u) / w, +inf unless 0 < w < inf (the + 0.0 turns the -0.0 of u == 1 into +0.0, which
// orders as its bits)
__device__ __forceinline__ double per_key(float p, double alpha, double u) {
    const double w = per_weight(p, alpha);
    if (!(w > 0.0 && w < __builtin_huge_val())) return __builtin_huge_val();
    return -log(u) / w + 0.0;
}

// The keys of items 4q .. 4q + 3 (+inf past size): Philox block m = i >> 1 serves items 2m, 2m + 1.
__device__ __forceinline__ void quad_keys(const float* __restrict__ pri, int64_t size, bool vec, int64_t q, double alpha,
                                          uint32_t k0, uint32_t k1, uint32_t d0, uint32_t d1, double e[4]) {
    const int64_t i0 = 4 * q;
    float p[4];
    if (vec && i0 + 3 < size) {
        const float4 v = *reinterpret_cast<const float4*>(pri + i0);
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = i0 + k < size ? pri[i0 + k] : 0.f;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const u32x4 r = philox({(uint32_t)(2 * q + h), d0, d1, kTagPer}, k0, k1);
        e[2 * h] = per_key(p[2 * h], alpha, 1.0 - u01(r.x, r.y));
        e[2 * h + 1] = per_key(p[2 * h + 1], alpha, 1.0 - u01(r.z, r.w));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i0 + k >= size) e[k] = __builtin_huge_val();
}

__global__ __launch_bounds__(kPerBlock) void k_per_hist(const float* __restrict__ pri, int64_t size, int vec, double alpha,
                                                        uint32_t k0, uint32_t k1, uint32_t d0, uint32_t d1,
                                                        double* __restrict__ keys_out, uint32_t* __restrict__ hist) {
    __shared__ uint32_t lh[kBins];
    for (int b = threadIdx.x; b < kBins; b += kPerBlock) lh[b] = 0;
    __syncthreads();
    const int64_t nq = (size + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * kPerBlock + threadIdx.x; q < nq; q += (int64_t)gridDim.x * kPerBlock) {
        double e[4];
        quad_keys(pri, size, vec != 0, q, alpha, k0, k1, d0, d1, e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = 4 * q + k;
            if (i >= size) continue;
            if (keys_out) keys_out[i] = e[k];
            const uint64_t bits = (uint64_t)__double_as_longlong(e[k]);
            if (bits < kInfBits) atomicAdd(&lh[(uint32_t)(bits >> kBinShift)], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kBins; b += kPerBlock)
        if (lh[b]) atomicAdd(&hist[b], lh[b]);
}

// One workgroup: T = the first bin at which the running count reaches batch (the last bin, with
// every finite key below it, when there are fewer).  Thread t owns bins 4t .. 4t + 3.
__global__ __launch_bounds__(kPerBlock) void k_per_scan(const uint32_t* __restrict__ hist, int32_t batch,
                                                        uint32_t* __restrict__ ctrl) {
    __shared__ uint32_t s[kPerBlock];
    constexpr int kPer = kBins / kPerBlock;
    uint32_t h[kPer], own = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) { h[k] = hist[kPer * threadIdx.x + k]; own += h[k]; }
    s[threadIdx.x] = own;
    __syncthreads();
    for (int o = 1; o < kPerBlock; o <<= 1) {   // inclusive scan (sizes below 2^31: no overflow)
        const uint32_t add = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    const uint32_t total = s[kPerBlock - 1];
    uint32_t run = s[threadIdx.x] - own;
    const uint32_t want = (uint32_t)batch;
    if (run < want && s[threadIdx.x] >= want) {   // exactly one thread
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const uint32_t next = run + h[k];
            if (run < want && next >= want) { ctrl[kCtrlBin] = kPer * threadIdx.x + k; ctrl[kCtrlExpect] = next; }
            run = next;
        }
    }
    if (threadIdx.x == 0) {
        if (total < want) { ctrl[kCtrlBin] = kBins - 1; ctrl[kCtrlExpect] = total; }
        ctrl[kCtrlFinite] = total;
    }
}

__global__ __launch_bounds__(kPerBlock) void k_per_collect(const float* __restrict__ pri, int64_t size, int vec, double alpha,
                                                           uint32_t k0, uint32_t k1, uint32_t d0, uint32_t d1,
                                                           uint32_t* __restrict__ ctrl, uint64_t* __restrict__ ckey,
                                                           int32_t* __restrict__ cidx, uint32_t cap) {
    const uint32_t T = ctrl[kCtrlBin];
    const int64_t nq = (size + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * kPerBlock + threadIdx.x; q < nq; q += (int64_t)gridDim.x * kPerBlock) {
        double e[4];
        quad_keys(pri, size, vec != 0, q, alpha, k0, k1, d0, d1, e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t bits = (uint64_t)__double_as_longlong(e[k]);
            if (bits < kInfBits && (uint32_t)(bits >> kBinShift) <= T) {
                const uint32_t pos = atomicAdd(&ctrl[kCtrlCount], 1u);
                if (pos < cap) { ckey[pos] = bits; cidx[pos] = (int32_t)(4 * q + k); }
            }
        }
    }
}

__device__ __forceinline__ bool cand_after(uint64_t ka, int32_t ia, uint64_t kb, int32_t ib) {
    return ka > kb || (ka == kb && ia > ib);
}

__global__ __launch_bounds__(kPerBlock) void k_per_final(const float* __restrict__ pri, int32_t batch, double alpha,
                                                         double beta, const float* __restrict__ ring, int32_t width,
                                                         const uint32_t* __restrict__ ctrl,
                                                         const uint64_t* __restrict__ ckey,
                                                         const int32_t* __restrict__ cidx, uint32_t cap,
                                                         int64_t* __restrict__ indices, float* __restrict__ weights,
                                                         float* __restrict__ rows, int32_t* __restrict__ info) {
    __shared__ uint64_t skey[kCapMax];
    __shared__ int32_t sidx[kCapMax];
    __shared__ double smin[kPerBlock / 64];
    const uint32_t arrived = ctrl[kCtrlCount];
    const uint32_t n = arrived < cap ? arrived : cap;
    uint32_t P = 1;
    while (P < n) P <<= 1;                      // P <= cap <= kCapMax (cap is a power of two)
    for (uint32_t i = threadIdx.x; i < P; i += kPerBlock) {
        skey[i] = i < n ? ckey[i] : ~0ull;
        sidx[i] = i < n ? cidx[i] : 0x7FFFFFFF;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < P; i += kPerBlock) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint64_t ka = skey[i], kb = skey[l];
                    const int32_t ia = sidx[i], ib = sidx[l];
                    if (cand_after(ka, ia, kb, ib) == ((i & k) == 0)) {
                        skey[i] = kb; sidx[i] = ib;
                        skey[l] = ka; sidx[l] = ia;
                    }
                }
            }
            __syncthreads();
        }
    const uint32_t nsel = n < (uint32_t)batch ? n : (uint32_t)batch;
    // thread j: slot j (batch <= kPerBlock)
    const int j = threadIdx.x;
    const int32_t id = j < (int)nsel ? sidx[j] : -1;
    const double w = id >= 0 ? per_weight(pri[id], alpha) : __builtin_huge_val();
    // the weight of the largest (size w / sum w)^-beta: the smallest w (the largest for a negative beta)
    const bool neg = beta < 0.0;
    double m = id >= 0 && neg ? -w : w;
    for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(m, o); m = t < m ? t : m; }
    if ((threadIdx.x & 63) == 0) smin[threadIdx.x >> 6] = m;
    __syncthreads();
    double wref = smin[0];
    for (int k = 1; k < kPerBlock / 64; ++k) wref = smin[k] < wref ? smin[k] : wref;
    if (neg) wref = -wref;
    if (j < batch) {
        indices[j] = id;
        weights[j] = id >= 0 ? (float)pow(wref / w, beta) : 0.f;
    }
    if (rows) {
        const int64_t total = (int64_t)batch * width;
        for (int64_t e = threadIdx.x; e < total; e += kPerBlock) {
            const int64_t s = e / width, c = e - s * width;
            rows[e] = s < (int64_t)nsel ? ring[(int64_t)sidx[s] * width + c] : 0.f;
        }
    }
    if (threadIdx.x == 0) {
        const uint32_t fin = ctrl[kCtrlFinite];
        info[0] = (int32_t)nsel;
        info[1] = fin > 0x7FFFFFFFu ? 0x7FFFFFFF : (int32_t)fin;
        info[2] = (arrived > cap || ctrl[kCtrlExpect] > cap) ? 1 : 0;
        info[3] = 0;
    }
}

__global__ __launch_bounds__(256) void k_per_update(float* __restrict__ pri, int64_t size,
                                                    const int64_t* __restrict__ indices,
                                                    const float* __restrict__ td, int32_t batch, float epsilon,
                                                    float* __restrict__ max_priority) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= batch) return;
    const int64_t i = indices[j];
    if (i < 0 || i >= size) return;
    const float p = fabsf(td[j]) + epsilon;
    pri[i] = p;
    // max(old, p) on non-negative floats = integer max of the bit patterns; a NaN compares false
    if (p > 0.f) atomicMax(reinterpret_cast<int*>(max_priority), __float_as_int(p));
}

}  // namespace

namespace pd {
pd_status set_error(pd_status s, const char* m);   // pdenv.hip: the pd_last_error() message
}

extern "C" {

size_t pd_per_sample_scratch_bytes(int64_t size, int32_t batch) {
    (void)size;   // (the keys are recomputed, not stored: nothing grows with the ring)
    const int32_t b = batch < 1 ? 1 : (batch > PD_PER_MAX_BATCH ? PD_PER_MAX_BATCH : batch);
    return kOffKeys + (size_t)per_capacity(b) * (sizeof(uint64_t) + sizeof(int32_t));
}

pd_status pd_per_sample(const float* priorities, int64_t size, int32_t batch, double alpha, double beta, uint64_t seed,
                        uint64_t draw, const float* ring, int32_t width, int64_t* indices, float* weights, float* rows,
                        double* keys_out, int32_t* info, void* scratch, size_t scratch_bytes, void* stream) {
    if (!priorities || !indices || !weights || !info || !scratch)
        return set_error(PD_ERR_INVALID, "pd_per_sample: null priorities, indices, weights, info or scratch");
    if (size < 1 || batch < 1 || batch > size)
        return set_error(PD_ERR_INVALID, "pd_per_sample: size >= 1 and 1 <= batch <= size are required");
    if ((rows && !ring) || (ring && width < 1))
        return set_error(PD_ERR_INVALID, "pd_per_sample: rows need a ring, a ring needs width >= 1");
    if (!(alpha >= 0.0) || !(alpha < __builtin_huge_val()) || !(beta > -__builtin_huge_val() && beta < __builtin_huge_val()))
        return set_error(PD_ERR_INVALID, "pd_per_sample: alpha must be finite and >= 0, beta finite");
    if (batch > PD_PER_MAX_BATCH) return set_error(PD_ERR_UNSUPPORTED, "pd_per_sample: batch above PD_PER_MAX_BATCH");
    if (size >= (1ll << 31)) return set_error(PD_ERR_UNSUPPORTED, "pd_per_sample: size must be below 2^31");
    if (scratch_bytes < pd_per_sample_scratch_bytes(size, batch) || (uintptr_t)scratch % 8 != 0)
        return set_error(PD_ERR_INVALID, "pd_per_sample: scratch too small or not 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const uint32_t cap = (uint32_t)per_capacity(batch);
    uint32_t* hist = (uint32_t*)scratch;
    uint32_t* ctrl = (uint32_t*)((char*)scratch + kOffCtrl);
    uint64_t* ckey = (uint64_t*)((char*)scratch + kOffKeys);
    int32_t* cidx = (int32_t*)(ckey + cap);
    const int vec = (uintptr_t)priorities % 16 == 0;
    const int64_t nq = (size + 3) / 4;
    const int64_t want = (nq + kPerBlock - 1) / kPerBlock;
    const unsigned grid = (unsigned)(want < kPerMaxGrid ? want : kPerMaxGrid);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), d0 = (uint32_t)draw, d1 = (uint32_t)(draw >> 32);
    if (hipMemsetAsync(scratch, 0, kOffKeys, s) != hipSuccess) return set_error(PD_ERR_HIP, "pd_per_sample: memset failed");
    hipLaunchKernelGGL(k_per_hist, dim3(grid), dim3(kPerBlock), 0, s, priorities, size, vec, alpha, k0, k1, d0, d1,
                       keys_out, hist);
    hipLaunchKernelGGL(k_per_scan, dim3(1), dim3(kPerBlock), 0, s, hist, batch, ctrl);
    hipLaunchKernelGGL(k_per_collect, dim3(grid), dim3(kPerBlock), 0, s, priorities, size, vec, alpha, k0, k1, d0, d1,
                       ctrl, ckey, cidx, cap);
    hipLaunchKernelGGL(k_per_final, dim3(1), dim3(kPerBlock), 0, s, priorities, batch, alpha, beta, rows ? ring : nullptr,
                       width, ctrl, ckey, cidx, cap, indices, weights, rows, info);
    if (hipGetLastError() != hipSuccess) return set_error(PD_ERR_HIP, "pd_per_sample: launch failed");
    return PD_OK;
}

pd_status pd_per_update(float* priorities, int64_t size, const int64_t* indices, const float* td_errors, int32_t batch,
                        float epsilon, float* max_priority, void* stream) {
    if (!priorities || !indices || !td_errors || !max_priority || size < 1 || batch < 0)
        return set_error(PD_ERR_INVALID, "pd_per_update: bad arguments");
    if (batch == 0) return PD_OK;
    hipLaunchKernelGGL(k_per_update, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, priorities,
                       size, indices, td_errors, batch, epsilon, max_priority);
    if (hipGetLastError() != hipSuccess) return set_error(PD_ERR_HIP, "pd_per_update: launch failed");
    return PD_OK;
}

}  // extern "C"
