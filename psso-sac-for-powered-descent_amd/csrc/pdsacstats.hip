// pdsacstats.hip -- the learning statistics of SACPyTorch._track_learning_stats (sac_pytorch.py:553-634)
// as ONE launch on device pointers: the 37 columns of a learning_stats row (the reference's key order,
// sac_pytorch.py:346-397) from the tensors a learner update leaves on the device, written as binary64
// into a caller's row.  Nothing is read back; the reference's own way is six device-to-host copies,
// four .item() calls and about thirty NumPy reductions per update.
//
// A series is a flat list of float32 values: each state dimension over the batch, all batch x A action
// values, the reward column, fminf(q1, q2), target_q, log_prob and the PER weights.  Every value is
// widened to binary64 and every sum is binary64 and two-pass (the mean, then the central moments about
// it: the cancellation of the one-pass formulas m2 = E[x^2] - mean^2 would cost digits the reference's
// float32 NumPy keeps).  A NaN in a series makes all its statistics NaN, min and max too (NumPy's
// behaviour), by a flag next to the comparisons.
//
// Layout: seven workgroups of 1024 threads, none of which reads what another writes -- each owns its
// columns of the row, so there is no counter, no scratch and no ordering between workgroups:
//   0  the S <= 16 state dimensions, one WAVE per dimension (lane l takes rows l, l + 64, ...; the row
//      pitch makes the loads strided, but the rows are few and L2-resident), the per-dimension
//      statistics through LDS, their plain mean over the dimensions by thread 0; and the scalar columns
//   1..5 action, reward, q, target_q, log_prob: the workgroup's 1024 lanes stride over the series,
//      wave64 butterfly, then the 16 wave partials through LDS, added in wave order by every thread
//   6  the PER columns (the mean of the weights)
// The summation order is fixed by the shape: element i belongs to lane i mod P (P = 64 or 1024), a lane
// adds its elements in ascending order, the xor butterfly adds pairs (a + b == b + a bit for bit, so
// every lane holds the same sum), the wave partials are added in ascending wave order.  No atomics.
#include <hip/hip_runtime.h>

#include "../../include/pdenv.h"

namespace {

constexpr int kStatBlock = 1024;
constexpr int kStatWaves = kStatBlock / 64;
constexpr int kStatGrid = 7;
constexpr int kMaxBatch = 65536;
// columns (sac_pytorch.py:346-397)
enum {
    kColStep = 0, kColState = 1, kColAction = 6, kColReward = 11, kColCriticLoss = 16, kColActorLoss = 17,
    kColAlphaLoss = 18, kColAlpha = 19, kColQ = 20, kColLogProb = 24, kColTargetQ = 28, kColPerBeta = 32,
    kColPerWeight = 33, kColPerMaxPrio = 34, kColActorNorm = 35, kColCriticNorm = 36
};
static_assert(kColCriticNorm + 1 == PD_SAC_N_STATS, "the columns of a learning_stats row");

const char* const kStatNames[PD_SAC_N_STATS] = {
    "step",
    "state_mean", "state_min", "state_max", "state_std", "state_kurtosis",
    "action_mean", "action_min", "action_max", "action_std", "action_kurtosis",
    "reward_mean", "reward_min", "reward_max", "reward_std", "reward_kurtosis",
    "critic_loss", "actor_loss", "alpha_loss", "alpha_value",
    "q_value_mean", "q_value_min", "q_value_max", "q_value_std",
    "log_prob_mean", "log_prob_min", "log_prob_max", "log_prob_std",
    "target_q_mean", "target_q_min", "target_q_max", "target_q_std",
    "per_beta", "per_mean_weight", "per_max_priority",
    "actor_grad_norm", "critic_grad_norm"};

struct StatArgs {
    int32_t batch, S, A, width;
    const float* rows;
    const float* q;
    const float* target_q;
    const float* log_prob;
    const float* weights;
    const float* critic_loss;
    const float* actor_loss;
    const float* alpha_loss;
    const float* log_alpha;
    const float* max_priority;
    const float* actor_grad_norm;
    const float* critic_grad_norm;
    double per_beta, step;
    double* out;
};

// Element i of a series of `inner` values per row at row pitch `pitch` (pair: fminf of the row's two).
__device__ __forceinline__ float stat_elem(const float* __restrict__ base, uint32_t i, uint32_t inner, uint32_t pitch,
                                           bool pair) {
    if (pair) return fminf(base[2 * (size_t)i], base[2 * (size_t)i + 1]);
    const uint32_t r = i / inner, c = i - r * inner;
    return base[(size_t)r * pitch + c];
}

__device__ __forceinline__ double wave_add(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// mean, min, max, std, kurtosis of a series of n >= 1 values into st[5], in every taking-part thread.
// wg: the whole workgroup reduces the series (every thread of it must call, `red` is its LDS
// exchange); otherwise the calling wave alone.  moments = false: the mean, min and max only.
__device__ __forceinline__ void series_stats(const float* __restrict__ base, uint32_t n, uint32_t inner, uint32_t pitch, bool pair, bool wg,
                             bool moments, double (*red)[4], double st[5]) {
    const uint32_t P = wg ? kStatBlock : 64, p = wg ? threadIdx.x : (threadIdx.x & 63);
    const int wave = threadIdx.x >> 6;
    const double nan = __builtin_nan("");
    double sum = 0.0;
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
    int bad = 0;
    for (uint32_t i = p; i < n; i += P) {
        const float x = stat_elem(base, i, inner, pitch, pair);
        sum += (double)x;
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
        bad |= x != x;
    }
    sum = wave_add(sum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    bad = __any(bad);
    double dmn = (double)mn, dmx = (double)mx, dbad = bad ? 1.0 : 0.0;
    if (wg) {
        if ((threadIdx.x & 63) == 0) { red[wave][0] = sum; red[wave][1] = dmn; red[wave][2] = dmx; red[wave][3] = dbad; }
        __syncthreads();
        sum = red[0][0]; dmn = red[0][1]; dmx = red[0][2]; dbad = red[0][3];
        for (int w = 1; w < kStatWaves; ++w) {
            sum += red[w][0];
            dmn = red[w][1] < dmn ? red[w][1] : dmn;
            dmx = red[w][2] > dmx ? red[w][2] : dmx;
            dbad += red[w][3];
        }
        __syncthreads();   // (red is written again below)
    }
    const double mean = sum / (double)n;
    st[0] = mean;
    st[1] = dbad != 0.0 ? nan : dmn;
    st[2] = dbad != 0.0 ? nan : dmx;
    st[3] = st[4] = nan;
    if (!moments) return;
    double m2 = 0.0, m4 = 0.0;
    for (uint32_t i = p; i < n; i += P) {
        const double d = (double)stat_elem(base, i, inner, pitch, pair) - mean;
        const double d2 = d * d;
        m2 += d2;
        m4 += d2 * d2;
    }
    m2 = wave_add(m2);
    m4 = wave_add(m4);
    if (wg) {
        if ((threadIdx.x & 63) == 0) { red[wave][0] = m2; red[wave][1] = m4; }
        __syncthreads();
        m2 = red[0][0]; m4 = red[0][1];
        for (int w = 1; w < kStatWaves; ++w) { m2 += red[w][0]; m4 += red[w][1]; }
    }
    m2 /= (double)n;
    m4 /= (double)n;
    st[3] = sqrt(m2);
    st[4] = m4 / (m2 * m2) - 3.0;   // Fisher, biased (scipy.stats.kurtosis); 0 / 0 = NaN for a constant series
}

__device__ __forceinline__ double scalar_or_nan(const float* p) { return p ? (double)*p : __builtin_nan(""); }

__global__ __launch_bounds__(kStatBlock) void k_sac_learning_stats(StatArgs t) {
    __shared__ double red[kStatWaves][4];
    __shared__ double dims[16][5];
    const uint32_t B = (uint32_t)t.batch, S = (uint32_t)t.S, A = (uint32_t)t.A, W = (uint32_t)t.width;
    double* __restrict__ out = t.out;
    const uint32_t wave = threadIdx.x >> 6;
    // the workgroup's series (one call site: the reduction's registers are not multiplied by inlining)
    const float* base = t.rows;
    uint32_t n = B, inner = 1, pitch = 1;
    bool pair = false, wg = true, moments = true, active = true;
    int col = 0, ncol = 0;
    switch (blockIdx.x) {
    case 0: base = t.rows + wave; pitch = W; wg = false; active = wave < S; break;
    case 1: base = t.rows + S; n = B * A; inner = A; pitch = W; col = kColAction; ncol = 5; break;
    case 2: base = t.rows + S + A; pitch = W; col = kColReward; ncol = 5; break;
    case 3: base = t.q; pair = true; col = kColQ; ncol = 4; break;
    case 4: base = t.target_q; col = kColTargetQ; ncol = 4; break;
    case 5: base = t.log_prob; col = kColLogProb; ncol = 4; break;
    default: base = t.weights; moments = false; active = t.weights != nullptr; col = kColPerWeight; ncol = 1; break;
    }
    double st[5];
    st[0] = st[1] = st[2] = st[3] = st[4] = __builtin_nan("");
    if (active) series_stats(base, n, inner, pitch, pair, wg, moments, red, st);
    if (blockIdx.x == 0) {
        if (active && (threadIdx.x & 63) == 0)
            for (int k = 0; k < 5; ++k) dims[wave][k] = st[k];
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 0; k < 5; ++k) {
                double s = dims[0][k];
                for (uint32_t d = 1; d < S; ++d) s += dims[d][k];
                out[kColState + k] = s / (double)S;
            }
            out[kColStep] = t.step;
            out[kColCriticLoss] = scalar_or_nan(t.critic_loss);
            out[kColActorLoss] = scalar_or_nan(t.actor_loss);
            out[kColAlphaLoss] = scalar_or_nan(t.alpha_loss);
            out[kColAlpha] = (double)expf(*t.log_alpha);
            out[kColActorNorm] = scalar_or_nan(t.actor_grad_norm);
            out[kColCriticNorm] = scalar_or_nan(t.critic_grad_norm);
        }
        return;
    }
    if (threadIdx.x == 0) {
        for (int k = 0; k < ncol; ++k) out[col + k] = st[k];
        if (blockIdx.x == kStatGrid - 1) {
            out[kColPerBeta] = t.weights ? t.per_beta : __builtin_nan("");
            out[kColPerMaxPrio] = scalar_or_nan(t.max_priority);
        }
    }
}

}  // namespace

namespace pd {
pd_status set_error(pd_status s, const char* m);   // pdenv.hip: the pd_last_error() message
}

extern "C" {

const char* pd_sac_stat_name(int32_t column) {
    return column >= 0 && column < PD_SAC_N_STATS ? kStatNames[column] : nullptr;
}

pd_status pd_sac_learning_stats(int64_t batch, int32_t state_dim, int32_t action_dim, const float* rows, int32_t width,
                                const float* q, const float* target_q, const float* log_prob, const float* weights,
                                const float* critic_loss, const float* actor_loss, const float* alpha_loss,
                                const float* log_alpha, const float* max_priority, const float* actor_grad_norm,
                                const float* critic_grad_norm, double per_beta, int64_t step, double* out_row,
                                void* stream) {
    using pd::set_error;
    if (batch < 1 || state_dim < 1 || action_dim < 1)
        return set_error(PD_ERR_INVALID, "pd_sac_learning_stats: batch, state_dim and action_dim >= 1 are required");
    if ((int64_t)width < (int64_t)state_dim + action_dim + 1)
        return set_error(PD_ERR_INVALID, "pd_sac_learning_stats: width below state_dim + action_dim + 1");
    if (!rows || !q || !target_q || !log_prob || !log_alpha || !out_row)
        return set_error(PD_ERR_INVALID, "pd_sac_learning_stats: null rows, q, target_q, log_prob, log_alpha or out_row");
    if (state_dim > 16 || action_dim > 8)
        return set_error(PD_ERR_UNSUPPORTED, "pd_sac_learning_stats: state_dim <= 16 and action_dim <= 8 are supported");
    if (batch > kMaxBatch) return set_error(PD_ERR_UNSUPPORTED, "pd_sac_learning_stats: batch above 65536");
    StatArgs t;
    t.batch = (int32_t)batch; t.S = state_dim; t.A = action_dim; t.width = width;
    t.rows = rows; t.q = q; t.target_q = target_q; t.log_prob = log_prob; t.weights = weights;
    t.critic_loss = critic_loss; t.actor_loss = actor_loss; t.alpha_loss = alpha_loss; t.log_alpha = log_alpha;
    t.max_priority = max_priority; t.actor_grad_norm = actor_grad_norm; t.critic_grad_norm = critic_grad_norm;
    t.per_beta = per_beta; t.step = (double)step; t.out = out_row;
    hipLaunchKernelGGL(k_sac_learning_stats, dim3(kStatGrid), dim3(kStatBlock), 0, (hipStream_t)stream, t);
    if (hipGetLastError() != hipSuccess) return set_error(PD_ERR_HIP, "pd_sac_learning_stats: launch failed");
    return PD_OK;
}

}  // extern "C"
