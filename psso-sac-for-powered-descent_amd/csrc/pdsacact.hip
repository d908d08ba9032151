// pdsacact.hip -- the last third of the SAC update on the device: the actor and temperature steps
// of SACPyTorch.update (sac_pytorch.py:485-521) -- actor.sample(states), critic(states,
// new_actions), min(q1, q2), the actor loss, zero_grad() + backward() through both critics into the
// actor, and the temperature loss's gradient -- as three launches; clip_grad_norm_ and the two
// Adam steps are pd_adam_step's (pdsacupd.hip).  No env handle: device pointers, the current HIP
// device, no host synchronisation, nothing read back, no float atomics: every sum has a fixed order.
//
//   pd_sac_critic_dinput  k_critic_dinput, grid (row tiles, 2 nets) as k_sac_critic: the forward pass
//                         on sac_mlp_tile (q is pd_sac_critic's bits); at the end of each layer's
//                         phase the signs of its post-ReLU tile are packed into LDS, one bit an
//                         activation (a wave ballot per 64 columns), which is all the backward chain
//                         with unit upstream gradient needs: delta_{L-1} = wm (h_{L-1} > 0), the
//                         hidden chain of pd_sac_bwd.h with no delta stored, then d q / d input_c =
//                         sum_j delta_0[j] W1[j][c] by the head stage's split (16 lanes a row, H / 16
//                         consecutive j each in ascending fma order, a shuffle tree over the parts).
//   pd_sac_actor_grad     pass a, k_actor_fwd, grid (row tiles, 2 nets): BOTH workgroups of a pair run
//                         the actor and the sample for their 16 rows (redundant, the same bits; the
//                         first of the pair writes the outputs, the actor's post-ReLU tiles and the
//                         rows' heads, eps and log_prob to scratch), then each runs its own Q net on
//                         state | new_action forward and, as above, backward to the action columns.
//                         At B = 256 that is 32 workgroups on 32 of 256 CUs either way, by the
//                         argument at the head of pdsactd.hip.
//                         pass b, k_actor_bwd, grid (row tiles): joins the two nets -- the loss
//                         coefficients, the sample's elementwise backward, dLoss / d(mean | raw
//                         log_std) -- leaves the tile's loss partials, and runs the actor's backward
//                         chain: delta_{L-1} from the two heads' weights, then pd_sac_bwd.h's, every
//                         delta to scratch.
//                         pass c, k_actor_wgrad, grid (output tiles of every actor layer): as
//                         k_critic_wgrad, the batch rows added in ascending order on MFMA; the two
//                         heads' dW are ONE row tile of 2A <= 16 rows against h_{L-1}.  Overwrites the
//                         caller's gradient tensors, leaves one sum of squares a workgroup, and adds
//                         the tiles' loss partials in tile order into actor_loss, log_alpha_grad and
//                         alpha_loss.
//
// Why three launches: the sample's backward needs both nets' dq/da of a row (a join over the pair),
// dW needs every row's delta (a join over the row tiles), and a launch boundary is the join that
// needs no memory of the library's own and no spinning workgroup (pdsacupd.hip's argument).
#include <hip/hip_runtime.h>

#include "../../include/pdenv.h"
#include "pd_common.h"
#include "pd_sac_bwd.h"

namespace {

using namespace pd;

constexpr int kMaxIn = 16;     // state_dim + action_dim of a Q net (sac_mlp_tile's layer 1: K <= 16)
constexpr int kHeadPitch = 16; // a row's heads (and their gradients): mean at k, log_std at 8 + k in LDS

struct QPair { SacQNet q[2]; };

__host__ __device__ inline int64_t pad16(int64_t b) { return (b + 15) / 16 * 16; }

// workgroups of pass c: layer 1 (4 row tiles of dW each), the hidden layers (a row tile by 128
// columns each), the two heads (128 columns each) -- k_critic_wgrad's split
__host__ __device__ inline int wg_layer1(int H) { return H / 64; }
__host__ __device__ inline int wg_hidden(int H) { return (H / 16) * (H / 128); }
__host__ __device__ inline int wg_head(int H) { return H / 128; }
__host__ __device__ inline int wg_net(int H, int L) { return wg_layer1(H) + (L - 1) * wg_hidden(H) + wg_head(H); }

// scratch, in floats, Bp = 16 ceil(batch / 16) rows: act [La][Bp][Ha], delta [La][Bp][Ha], dheads
// [Bp][16], heads [Bp][2A], eps [Bp][A], dqda [Bp][2][A], q [Bp][2], lp [Bp], loss partials [Bp / 16][2]
struct Scratch {
    float* act; float* delta; float* dh; float* heads; float* eps; float* dqda; float* q; float* lp; float* lpart;
};

size_t scratch_floats(int64_t batch, int32_t A, int32_t H, int32_t L) {
    const int64_t bp = pad16(batch);
    return (size_t)(bp * (2 * (int64_t)L * H + 5 * (int64_t)A + 19) + bp / 8);
}

// pdsactd.hip's gauss_pair_nt: gauss_pair (pd_common.h) with pd_log in place of the handle's log table
__device__ __forceinline__ void gauss_pair_nt(u32x4 r, double& z0, double& z1) {
    const double u1 = 1.0 - u01(r.x, r.y), u2 = u01(r.z, r.w);
    const double rho = sqrt(-2.0 * pd_log(u1));
    double s, c;
    sincos_fd(6.283185307179586 * u2, s, c);
    z0 = rho * c;
    z1 = rho * s;
}

// The signs of a post-ReLU tile src [16][H + 4] (LDS) as bits dst [16][H / 32]: a wave takes 64
// consecutive columns of a row per round
template <int H>
__device__ __forceinline__ void pack_signs(const float* src, uint32_t* dst) {
    constexpr int P = H + 4;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < kSacTile * H; i += kSacBlock) {
        const int row = i / H, col = i - row * H;
        const uint64_t m = __ballot(src[row * P + col] > 0.f);
        if (lane == 0) {
            dst[row * (H / 32) + col / 32] = (uint32_t)m;
            dst[row * (H / 32) + col / 32 + 1] = (uint32_t)(m >> 32);
        }
    }
}

// d q / d input_c, c in [c0, c1), of the tile's 16 rows with unit upstream gradient, after the
// net's forward pass has left its layers' signs in mask [L][16][H / 32]; hb: the forward pass's
// LDS (free behind the caller's barrier).  out(e, c, v), by one lane a row and column.
template <int H, typename Out>
__device__ __forceinline__ void q_dinput(const SacQNet& net, float* hb, const uint32_t* mask, int c0, int c1, Out&& out) {
    constexpr int P = H + 4, MW = H / 32, KP = H / 16;
    const int tid = threadIdx.x;
    const int L = net.L, D = net.S;
    float* dcur = hb;
    float* dnxt = hb + kSacTile * P;
    auto pos = [&](int l, int row, int col) { return (mask[(l * kSacTile + row) * MW + (col >> 5)] >> (col & 31)) & 1u; };
    for (int i = tid; i < kSacTile * H; i += kSacBlock) {
        const int row = i / H, col = i - row * H;
        dcur[row * P + col] = pos(L - 1, row, col) ? net.wm[col] : 0.f;
    }
    __syncthreads();
    const float* d0 = sac_bwd_hidden<H>(net.w, L, dcur, dnxt, pos);
    const int e = tid >> 4, p = tid & 15;
    const float* dr = d0 + e * P + p * KP;
    const float* w1 = net.w[0] + (size_t)(p * KP) * D;
    for (int c = c0; c < c1; ++c) {
        float s = 0.f;
#pragma unroll 4
        for (int k = 0; k < KP; ++k) s = fmaf(dr[k], w1[k * D + c], s);
        s += __shfl_xor(s, 8, 16);
        s += __shfl_xor(s, 4, 16);
        s += __shfl_xor(s, 2, 16);
        s += __shfl_xor(s, 1, 16);
        if (p == 0) out(e, c, s);
    }
}

template <int H>
__global__ __launch_bounds__(kSacBlock) void k_critic_dinput(QPair nets, int64_t n, int D, int pitch,
                                                             const float* __restrict__ sa, float* __restrict__ q,
                                                             float* __restrict__ dsa) {
    __shared__ __attribute__((aligned(16))) float hb[sac_mlp_lds_floats<H>()];
    __shared__ float s_sa[kSacTile * kMaxIn];
    __shared__ uint32_t s_mask[kSacMaxLayers * kSacTile * (H / 32)];
    constexpr int P = H + 4;
    const int tid = threadIdx.x;
    const int which = blockIdx.y;
    const SacQNet& net = nets.q[which];
    const int L = net.L;
    const int64_t e0 = (int64_t)blockIdx.x * kSacTile;
    if (tid < kSacTile * D) {
        const int te = tid / D, c = tid - te * D;
        const int64_t ge = e0 + te;
        s_sa[tid] = ge < n ? sa[ge * pitch + c] : 0.f;
    }
    __syncthreads();
    sac_mlp_tile<H>(net, n, e0, hb, [&](int e, int, float v) {
        const int64_t ge = e0 + e;
        if (q && ge < n) q[ge * 2 + which] = v;
    }, [&](int k) {
        if (k < L) pack_signs<H>((k & 1) ? hb + kSacTile * P : hb, s_mask + k * kSacTile * (H / 32));
    }, s_sa);
    __syncthreads();
    q_dinput<H>(net, hb, s_mask, 0, D, [&](int e, int c, float v) {
        const int64_t ge = e0 + e;
        if (dsa && ge < n) dsa[(ge * 2 + which) * D + c] = v;
    });
}

struct FwdArgs {
    SacMlp actor;
    QPair critic;
    Scratch s;
    const float* rows;
    int64_t n;
    int32_t S, A, pitch, has_critic;
    float lo, hi, max_action;
    uint32_t k0, k1, d0, d1;
    const float* eps_in;
    float* new_actions;
    float* log_prob;
    float* q;
    float* heads;
    float* eps_out;
    float* dq_da;
};

template <int HA, int HC>
__global__ __launch_bounds__(kSacBlock) void k_actor_fwd(FwdArgs t) {
    constexpr int HM = HA > HC ? HA : HC;
    __shared__ __attribute__((aligned(16))) float hb[sac_mlp_lds_floats<HM>()];
    __shared__ float s_st[kSacTile * kMaxIn];          // state [16][S]: the actor's observations
    __shared__ float s_sa[kSacTile * kMaxIn];          // state | new_action [16][S + A]: the critic's (S + A <= 16 with one)
    __shared__ float s_heads[kSacTile * kHeadPitch];
    __shared__ float s_lp[kSacTile * 8];
    __shared__ uint32_t s_mask[kSacMaxLayers * kSacTile * (HC / 32)];
    const int tid = threadIdx.x;
    const int S = t.S, A = t.A, D = S + A;
    const int which = blockIdx.y;
    const bool first = which == 0;
    const int64_t n = t.n, bp = pad16(n);
    const int64_t e0 = (int64_t)blockIdx.x * kSacTile;
    const int La = t.actor.L;
    if (tid < kSacTile * S) {
        const int te = tid / S, c = tid - te * S;
        const int64_t ge = e0 + te;
        const float v = ge < n ? t.rows[ge * t.pitch + c] : 0.f;
        s_st[tid] = v;
        if (t.has_critic) s_sa[te * D + c] = v;      // (without a critic S + A may exceed s_sa's 16 columns)
    }
    __syncthreads();
    // ---- heads = Actor.forward(state), pd_sac_actor's bits; the layers' post-ReLU tiles to act[k]
    sac_mlp_tile<HA>(t.actor, n, e0, hb, [&](int e, int o, float v) {
        s_heads[e * kHeadPitch + (o < A ? o : 8 + (o - A))] = v;
        const int64_t ge = e0 + e;
        if (first) {
            t.s.heads[ge * 2 * A + o] = v;
            if (t.heads && ge < n) t.heads[ge * 2 * A + o] = v;
        }
    }, [&](int k) {
        if (!first || k >= La) return;
        constexpr int PA = HA + 4;
        const float* src = (k & 1) ? hb + kSacTile * PA : hb;
        float* dst = t.s.act + ((size_t)k * bp + e0) * HA;
        for (int i = tid; i < kSacTile * (HA / 4); i += kSacBlock) {
            const int row = i / (HA / 4), c4 = i - row * (HA / 4);
            *(f32x4*)(dst + (size_t)row * HA + 4 * c4) = *(const f32x4*)(src + row * PA + 4 * c4);
        }
    }, s_st);
    __syncthreads();
    // ---- eps, the sampled action and the log-probability's terms, pd_sac_td_target's expressions:
    // thread (row te, component k)
    {
        const int te = tid >> 4, k = tid & 15;
        const int64_t ge = e0 + te;
        if (k < A) {
            const float m = s_heads[te * kHeadPitch + k];
            float ls = s_heads[te * kHeadPitch + 8 + k];
            ls = ls < t.lo ? t.lo : (ls > t.hi ? t.hi : ls);
            const float sd = expf(ls);
            float ek = 0.f;
            if (ge < n) {
                if (t.eps_in) ek = t.eps_in[ge * A + k];
                else {
                    const u32x4 r = philox({(uint32_t)ge, t.d0, t.d1, kTagActEps + (uint32_t)(k >> 1)}, t.k0, t.k1);
                    double z0, z1;
                    gauss_pair_nt(r, z0, z1);
                    ek = (float)((k & 1) ? z1 : z0);
                }
            }
            const float x = m + sd * ek;
            const float a = tanhf(x);
            const float act = a * t.max_action;
            const float d = x - m;
            const float lp = -(d * d) / (2.f * (sd * sd)) - ls - 0.9189385332046727f - logf(1.f - a * a + 1e-6f);
            s_lp[te * 8 + k] = lp;
            if (t.has_critic) s_sa[te * D + S + k] = act;
            if (first) {
                t.s.eps[ge * A + k] = ek;
                if (ge < n) {
                    if (t.eps_out) t.eps_out[ge * A + k] = ek;
                    if (t.new_actions) t.new_actions[ge * A + k] = act;
                }
            }
        }
    }
    __syncthreads();
    if (first && tid < kSacTile) {
        const int64_t ge = e0 + tid;
        float lp = s_lp[tid * 8];
        for (int k = 1; k < A; ++k) lp += s_lp[tid * 8 + k];
        t.s.lp[ge] = lp;
        if (t.log_prob && ge < n) t.log_prob[ge] = lp;
    }
    if (!t.has_critic) return;
    // ---- this workgroup's Q net on state | new_action, pd_sac_critic's bits, and its gradient with
    // respect to the action columns
    const SacQNet& net = t.critic.q[which];
    const int Lc = net.L;
    sac_mlp_tile<HC>(net, n, e0, hb, [&](int e, int, float v) {
        const int64_t ge = e0 + e;
        t.s.q[ge * 2 + which] = v;
        if (t.q && ge < n) t.q[ge * 2 + which] = v;
    }, [&](int k) {
        constexpr int PC = HC + 4;
        if (k < Lc) pack_signs<HC>((k & 1) ? hb + kSacTile * PC : hb, s_mask + k * kSacTile * (HC / 32));
    }, s_sa);
    __syncthreads();
    q_dinput<HC>(net, hb, s_mask, S, D, [&](int e, int c, float v) {
        const int64_t ge = e0 + e;
        t.s.dqda[(ge * 2 + which) * A + (c - S)] = v;
        if (t.dq_da && ge < n) t.dq_da[(ge * 2 + which) * A + (c - S)] = v;
    });
}

struct BwdArgs {
    SacMlp actor;
    Scratch s;
    int64_t n;
    int32_t A, has_critic;
    float lo, hi, max_action, target_entropy;
    const float* log_alpha;
    const float* weights;
    const float* dheads_in;
    float* dheads_out;
};

template <int H>
__global__ __launch_bounds__(kSacBlock) void k_actor_bwd(BwdArgs t) {
    constexpr int P = H + 4;
    __shared__ __attribute__((aligned(16))) float hb[2 * kSacTile * P];
    __shared__ float s_dh[kSacTile * kHeadPitch];      // dLoss / d mean at k, / d raw log_std at 8 + k
    __shared__ float s_la[kSacTile], s_lt[kSacTile];
    const int tid = threadIdx.x;
    const int A = t.A, L = t.actor.L;
    const int64_t n = t.n, bp = pad16(n);
    const int64_t e0 = (int64_t)blockIdx.x * kSacTile;
    const float bf = (float)n;
    s_dh[tid] = 0.f;
    __syncthreads();
    // ---- the join of the two nets and the sample's backward: thread (row te, component k)
    {
        const int te = tid >> 4, k = tid & 15;
        const int64_t ge = e0 + te;
        if (k < A && ge < n) {
            float dm, dr;
            if (t.dheads_in) {
                dm = t.dheads_in[ge * 2 * A + k];
                dr = t.dheads_in[ge * 2 * A + A + k];
            } else {
                const float m = t.s.heads[ge * 2 * A + k], raw = t.s.heads[ge * 2 * A + A + k];
                const float ls = raw < t.lo ? t.lo : (raw > t.hi ? t.hi : raw);
                const float sd = expf(ls);
                const float ek = t.s.eps[ge * A + k];
                const float x = m + sd * ek;
                const float a = tanhf(x);
                const float w = t.weights ? t.weights[ge] : 1.f;
                const float alpha = expf(*t.log_alpha);
                const float q1 = t.s.q[ge * 2], q2 = t.s.q[ge * 2 + 1];
                // torch.min's backward: the smaller takes the gradient, a tie halves it
                const float sel1 = q1 < q2 ? 1.f : (q1 > q2 ? 0.f : 0.5f);
                const float sel2 = q2 < q1 ? 1.f : (q2 > q1 ? 0.f : 0.5f);
                const float wb = w / bf;
                const float c1 = -(wb * sel1), c2 = -(wb * sel2);
                const float cl = (w * alpha) / bf;
                const float g = c1 * t.s.dqda[(ge * 2) * A + k] + c2 * t.s.dqda[(ge * 2 + 1) * A + k];
                const float tt = 1.f - a * a;
                const float gx = (g * t.max_action) * tt + cl * (((2.f * a) * tt) / (tt + 1e-6f));
                dm = gx;
                dr = (raw >= t.lo && raw <= t.hi) ? (gx * sd) * ek - cl : 0.f;
            }
            s_dh[te * kHeadPitch + k] = dm;
            s_dh[te * kHeadPitch + 8 + k] = dr;
            if (t.dheads_out) {
                t.dheads_out[ge * 2 * A + k] = dm;
                t.dheads_out[ge * 2 * A + A + k] = dr;
            }
        }
    }
    // ---- the rows' loss terms: thread te, row e0 + te
    if (tid < kSacTile) {
        const int64_t ge = e0 + tid;
        float la = 0.f, lt = 0.f;
        if (ge < n) {
            const float w = t.weights ? t.weights[ge] : 1.f;
            const float lp = t.s.lp[ge];
            lt = w * (lp + t.target_entropy);
            if (t.has_critic) {
                const float alpha = expf(*t.log_alpha);
                la = w * (alpha * lp - fminf(t.s.q[ge * 2], t.s.q[ge * 2 + 1]));
            }
        }
        s_la[tid] = la;
        s_lt[tid] = lt;
    }
    __syncthreads();
    if (tid == 0) {
        float sa = s_la[0], st = s_lt[0];
        for (int k = 1; k < kSacTile; ++k) { sa += s_la[k]; st += s_lt[k]; }
        t.s.lpart[blockIdx.x * 2] = sa;
        t.s.lpart[blockIdx.x * 2 + 1] = st;
    }
    // the tile's head gradients as pass c's left operand: row tile rows 0 .. A - 1 mean, A .. 2A - 1 log_std
    {
        const int te = tid >> 4, o = tid & 15;
        t.s.dh[(e0 + te) * 16 + o] = o < A ? s_dh[te * kHeadPitch + o] : (o < 2 * A ? s_dh[te * kHeadPitch + 8 + (o - A)] : 0.f);
    }
    // ---- the heads' backward: delta_{L-1}[b][j] = (sum_k dmean_k Wm[k][j] + sum_k draw_k Ws[k][j])
    // (h_{L-1}[b][j] > 0), one fma chain, the mean head's terms first, k ascending
    const float* act = t.s.act;
    float* delta = t.s.delta;
    float* dcur = hb;
    float* dnxt = hb + kSacTile * P;
    {
        const float* hl = act + ((size_t)(L - 1) * bp + e0) * H;
        float* dl = delta + ((size_t)(L - 1) * bp + e0) * H;
        for (int i = tid; i < kSacTile * H; i += kSacBlock) {
            const int row = i / H, col = i - row * H;
            float s = 0.f;
            for (int k = 0; k < A; ++k) s = fmaf(s_dh[row * kHeadPitch + k], t.actor.wm[(size_t)k * H + col], s);
            for (int k = 0; k < A; ++k) s = fmaf(s_dh[row * kHeadPitch + 8 + k], t.actor.ws[(size_t)k * H + col], s);
            const float v = hl[(size_t)row * H + col] > 0.f ? s : 0.f;
            dcur[row * P + col] = v;
            dl[(size_t)row * H + col] = v;
        }
    }
    __syncthreads();
    sac_bwd_hidden<H>(t.actor.w, L, dcur, dnxt,
                      [&](int l, int row, int col) { return act[((size_t)l * bp + e0 + row) * H + col] > 0.f; },
                      [&](int l, int row, int col, float v) { delta[((size_t)l * bp + e0 + row) * H + col] = v; });
}

struct AGrad {
    float* w[kSacMaxLayers];
    float* b[kSacMaxLayers];
    float* wm; float* bm; float* ws; float* bs;
};

struct WArgs {
    AGrad g;
    Scratch s;
    int64_t n;
    int32_t S, A, pitch, L, has_critic;
    const float* rows;
    const float* log_alpha;
    float* actor_loss;
    float* alpha_loss;
    float* log_alpha_grad;
    float* sumsq;
};

template <int H>
__global__ __launch_bounds__(kSacBlock) void k_actor_wgrad(WArgs a) {
    __shared__ float s_ss[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q4 = lane >> 4;
    const int L = a.L, S = a.S, A = a.A;
    const int64_t n = a.n, bp = pad16(n);
    const AGrad& g = a.g;
    const float* act = a.s.act;
    const float* delta = a.s.delta;
    int x = blockIdx.x;
    float ss = 0.f;      // the squares of what this lane writes
    f32x4 accb;
    if (x < wg_layer1(H)) {
        // ---- layer 1: dW_1 [H][S] = delta_0^T . state, wave: row tile 4 x + wave
        const int j0 = 16 * (4 * x + wave);
        f32x4 acc[1];
        wave_wgrad<1>(bp, true,
                      [&](int64_t b0) { return delta[(size_t)(b0 + q4) * H + j0 + r]; },
                      [&](int64_t b0, int) { return (r < S && b0 + q4 < n) ? a.rows[(b0 + q4) * a.pitch + r] : 0.f; },
                      acc, accb);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int row = j0 + 4 * q4 + m;
            if (r < S) { g.w[0][(size_t)row * S + r] = acc[0][m]; ss += acc[0][m] * acc[0][m]; }
            if (r == 0) { g.b[0][row] = accb[m]; ss += accb[m] * accb[m]; }
        }
    } else if (x < wg_layer1(H) + (L - 1) * wg_hidden(H)) {
        // ---- hidden layer l: dW_l [H][H] = delta_l^T . h_{l-1}, workgroup: row tile jt, 128
        // columns from 128 kc, wave: 32 of them
        x -= wg_layer1(H);
        const int l = 1 + x / wg_hidden(H);
        const int rem = x % wg_hidden(H);
        const int j0 = 16 * (rem / (H / 128)), kc = rem % (H / 128);
        const int k0 = 128 * kc + 32 * wave;
        const bool bias = kc == 0 && wave == 0;
        const float* dl = delta + (size_t)l * bp * H;
        const float* hl = act + (size_t)(l - 1) * bp * H;
        f32x4 acc[2];
        wave_wgrad<2>(bp, bias,
                      [&](int64_t b0) { return dl[(size_t)(b0 + q4) * H + j0 + r]; },
                      [&](int64_t b0, int i) { return hl[(size_t)(b0 + q4) * H + k0 + 16 * i + r]; },
                      acc, accb);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int row = j0 + 4 * q4 + m;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                g.w[l][(size_t)row * H + k0 + 16 * i + r] = acc[i][m];
                ss += acc[i][m] * acc[i][m];
            }
            if (bias && r == 0) { g.b[l][row] = accb[m]; ss += accb[m] * accb[m]; }
        }
    } else {
        // ---- the two heads: [dWm ; dWs] [2A][H] = dheads^T . h_{L-1}, one row tile (rows past 2A are
        // zero and not written), the biases its column sums
        const int kc = x - wg_layer1(H) - (L - 1) * wg_hidden(H);
        const int k0 = 128 * kc + 32 * wave;
        const bool bias = kc == 0 && wave == 0;
        const float* hl = act + (size_t)(L - 1) * bp * H;
        const float* dh = a.s.dh;
        f32x4 acc[2];
        wave_wgrad<2>(bp, bias,
                      [&](int64_t b0) { return dh[(b0 + q4) * 16 + r]; },
                      [&](int64_t b0, int i) { return hl[(size_t)(b0 + q4) * H + k0 + 16 * i + r]; },
                      acc, accb);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int row = 4 * q4 + m;
            if (row < 2 * A) {
                float* dw = row < A ? g.wm + (size_t)row * H : g.ws + (size_t)(row - A) * H;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    dw[k0 + 16 * i + r] = acc[i][m];
                    ss += acc[i][m] * acc[i][m];
                }
                if (bias && r == 0) {
                    if (row < A) g.bm[row] = accb[m];
                    else g.bs[row - A] = accb[m];
                    ss += accb[m] * accb[m];
                }
            }
        }
    }
    // ---- this workgroup's sum of squares: a fixed tree over the lanes, then the waves in order
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if (lane == 0) s_ss[wave] = ss;
    __syncthreads();
    if (tid == 0 && a.sumsq) a.sumsq[blockIdx.x] = ((s_ss[0] + s_ss[1]) + s_ss[2]) + s_ss[3];
    // ---- the losses from the row tiles' partials, tile by tile, by one thread
    if (blockIdx.x == 0 && tid == 0) {
        float s1 = 0.f, s2 = 0.f;
        for (int64_t t = 0; t < bp / 16; ++t) { s1 += a.s.lpart[2 * t]; s2 += a.s.lpart[2 * t + 1]; }
        const float bf = (float)n;
        const float ga = -(s2 / bf);
        if (a.actor_loss && a.has_critic) a.actor_loss[0] = s1 / bf;
        if (a.log_alpha_grad) a.log_alpha_grad[0] = ga;
        if (a.alpha_loss) a.alpha_loss[0] = a.log_alpha[0] * ga;
    }
}

bool hidden_ok(int32_t h) { return h == 128 || h == 256 || h == 512; }

// params (2 (L + 1) pointers, named_parameters() order) into a Q net; 0, or the status of the
// first defect: PD_ERR_INVALID for a null pointer, PD_ERR_UNSUPPORTED for a misaligned one
pd_status fill_qnet(SacQNet& q, int32_t in_dim, int32_t hidden, int32_t L, const float* const* p) {
    q.S = in_dim; q.L = L; q.A = 1; q.H = hidden; q.obs = nullptr;
    for (int k = 0; k < 2 * (L + 1); ++k)
        if (!p[k]) return PD_ERR_INVALID;
    for (int k = 0; k < 2 * (L + 1); ++k)
        if ((uintptr_t)p[k] % 16 != 0) return PD_ERR_UNSUPPORTED;
    for (int l = 0; l < L; ++l) { q.w[l] = p[2 * l]; q.b[l] = p[2 * l + 1]; }
    q.wm = p[2 * L]; q.bm = p[2 * L + 1];
    q.ws = q.wm; q.bs = q.bm;      // (never read: one head)
    return PD_OK;
}

}  // namespace

namespace pd {
pd_status set_error(pd_status s, const char* m);   // pdenv.hip: the pd_last_error() message
}

extern "C" {

pd_status pd_sac_critic_dinput(int64_t batch, int32_t state_dim, int32_t action_dim, int32_t hidden,
                               int32_t n_hidden_layers, const float* sa, int32_t pitch, const float* const* params_q1,
                               const float* const* params_q2, float* q, float* dsa, void* stream) {
    const int64_t D = (int64_t)state_dim + action_dim;
    if (batch < 0 || state_dim < 1 || action_dim < 1 || D > kMaxIn || n_hidden_layers < 1 ||
        n_hidden_layers > kSacMaxLayers || !params_q1 || !params_q2 || (batch > 0 && !sa))
        return set_error(PD_ERR_INVALID, "pd_sac_critic_dinput: bad arguments");
    if (pitch < D) return set_error(PD_ERR_INVALID, "pd_sac_critic_dinput: pitch below state_dim + action_dim");
    if (!hidden_ok(hidden)) return set_error(PD_ERR_UNSUPPORTED, "pd_sac_critic_dinput: hidden width 128, 256 or 512 only");
    QPair nets{};
    const float* const* ps[2] = {params_q1, params_q2};
    for (int w = 0; w < 2; ++w) {
        const pd_status st = fill_qnet(nets.q[w], (int32_t)D, hidden, n_hidden_layers, ps[w]);
        if (st == PD_ERR_INVALID) return set_error(st, "pd_sac_critic_dinput: null layer parameter");
        if (st != PD_OK) return set_error(st, "pd_sac_critic_dinput: parameter not 16-byte aligned");
    }
    if (batch == 0) return PD_OK;
    if ((batch + kSacTile - 1) / kSacTile > 0x7FFFFFFFll)
        return set_error(PD_ERR_UNSUPPORTED, "pd_sac_critic_dinput: batch above 2^35");
    const dim3 grid((unsigned)((batch + kSacTile - 1) / kSacTile), 2);
    hipStream_t s = (hipStream_t)stream;
    switch (hidden) {
        case 128: hipLaunchKernelGGL(k_critic_dinput<128>, grid, dim3(kSacBlock), 0, s, nets, batch, (int)D, pitch, sa, q, dsa); break;
        case 512: hipLaunchKernelGGL(k_critic_dinput<512>, grid, dim3(kSacBlock), 0, s, nets, batch, (int)D, pitch, sa, q, dsa); break;
        default: hipLaunchKernelGGL(k_critic_dinput<256>, grid, dim3(kSacBlock), 0, s, nets, batch, (int)D, pitch, sa, q, dsa); break;
    }
    if (hipGetLastError() != hipSuccess) return set_error(PD_ERR_HIP, "pd_sac_critic_dinput: launch failed");
    return PD_OK;
}

size_t pd_sac_actor_grad_scratch_bytes(int64_t batch, int32_t action_dim, int32_t actor_hidden, int32_t actor_layers) {
    if (batch <= 0 || action_dim <= 0 || actor_hidden <= 0 || actor_layers <= 0) return 0;
    return 4 * scratch_floats(batch, action_dim, actor_hidden, actor_layers);
}

pd_status pd_sac_actor_grad(int64_t batch, int32_t state_dim, int32_t action_dim, const float* rows, int32_t pitch,
                            const float* weights, int32_t actor_hidden, int32_t actor_layers,
                            const float* const* actor_params, float* const* actor_grads, float log_std_min,
                            float log_std_max, float max_action, int32_t critic_hidden, int32_t critic_layers,
                            const float* const* params_q1, const float* const* params_q2, const float* log_alpha,
                            float target_entropy, uint64_t seed, uint64_t draw, const float* eps_in,
                            const float* dheads_in, float* new_actions, float* log_prob, float* q, float* heads,
                            float* eps_out, float* dq_da, float* dheads_out, float* actor_loss, float* alpha_loss,
                            float* log_alpha_grad, float* sumsq_partials, int32_t* n_partials, void* scratch,
                            size_t scratch_bytes, void* stream) {
    const bool has_critic = dheads_in == nullptr;
    const int32_t La = actor_layers;
    if (batch < 0 || state_dim < 1 || action_dim < 1 || !actor_params || !actor_grads || !log_alpha ||
        (has_critic && (!params_q1 || !params_q2)) || (batch > 0 && !rows))
        return set_error(PD_ERR_INVALID, "pd_sac_actor_grad: bad arguments");
    if (pitch < state_dim) return set_error(PD_ERR_INVALID, "pd_sac_actor_grad: pitch below state_dim");
    if (sumsq_partials && !n_partials)
        return set_error(PD_ERR_INVALID, "pd_sac_actor_grad: sumsq_partials without n_partials");
    if (state_dim > kMaxIn || action_dim > 8 || La < 1 || La > kSacMaxLayers ||
        (has_critic && (state_dim + (int64_t)action_dim > kMaxIn || critic_layers < 1 || critic_layers > kSacMaxLayers)))
        return set_error(PD_ERR_UNSUPPORTED, "pd_sac_actor_grad: state_dim <= 16, action_dim <= 8, state_dim + action_dim "
                                             "<= 16 for the critic, 1 to 8 hidden layers");
    if (!hidden_ok(actor_hidden) || (has_critic && !hidden_ok(critic_hidden)))
        return set_error(PD_ERR_UNSUPPORTED, "pd_sac_actor_grad: hidden width 128, 256 or 512 only");
    const int32_t need_partials = wg_net(actor_hidden, La);
    if (sumsq_partials && *n_partials < need_partials)
        return set_error(PD_ERR_INVALID, "pd_sac_actor_grad: sumsq_partials shorter than H / 64 + (L - 1) (H / 16) "
                                         "(H / 128) + H / 128");
    FwdArgs fa{};
    BwdArgs ba{};
    WArgs wa{};
    SacMlp& a = fa.actor;
    a.S = state_dim; a.L = La; a.A = action_dim; a.H = actor_hidden; a.obs = nullptr;
    for (int k = 0; k < 2 * (La + 2); ++k)
        if (!actor_params[k] || !actor_grads[k])
            return set_error(PD_ERR_INVALID, "pd_sac_actor_grad: null actor parameter or gradient");
    for (int k = 0; k < 2 * (La + 2); ++k)
        if ((uintptr_t)actor_params[k] % 16 != 0 || (uintptr_t)actor_grads[k] % 16 != 0)
            return set_error(PD_ERR_UNSUPPORTED, "pd_sac_actor_grad: parameter or gradient not 16-byte aligned");
    for (int l = 0; l < La; ++l) {
        a.w[l] = actor_params[2 * l]; a.b[l] = actor_params[2 * l + 1];
        wa.g.w[l] = actor_grads[2 * l]; wa.g.b[l] = actor_grads[2 * l + 1];
    }
    a.wm = actor_params[2 * La]; a.bm = actor_params[2 * La + 1];
    a.ws = actor_params[2 * La + 2]; a.bs = actor_params[2 * La + 3];
    wa.g.wm = actor_grads[2 * La]; wa.g.bm = actor_grads[2 * La + 1];
    wa.g.ws = actor_grads[2 * La + 2]; wa.g.bs = actor_grads[2 * La + 3];
    ba.actor = a;
    if (has_critic) {
        const float* const* ps[2] = {params_q1, params_q2};
        for (int w = 0; w < 2; ++w) {
            const pd_status st = fill_qnet(fa.critic.q[w], state_dim + action_dim, critic_hidden, critic_layers, ps[w]);
            if (st == PD_ERR_INVALID) return set_error(st, "pd_sac_actor_grad: null critic parameter");
            if (st != PD_OK) return set_error(st, "pd_sac_actor_grad: parameter not 16-byte aligned");
        }
    }
    if (batch == 0) {
        if (n_partials) *n_partials = 0;
        return PD_OK;
    }
    if ((batch + kSacTile - 1) / kSacTile > 0x7FFFFFFFll)
        return set_error(PD_ERR_UNSUPPORTED, "pd_sac_actor_grad: batch above 2^35");
    const size_t need = 4 * scratch_floats(batch, action_dim, actor_hidden, La);
    if (!scratch || scratch_bytes < need || (uintptr_t)scratch % 16 != 0)
        return set_error(PD_ERR_INVALID, "pd_sac_actor_grad: scratch missing, misaligned or shorter than "
                                         "pd_sac_actor_grad_scratch_bytes");
    const int64_t bp = pad16(batch);
    const int A = action_dim;
    Scratch s;
    s.act = (float*)scratch;
    s.delta = s.act + (size_t)La * bp * actor_hidden;
    s.dh = s.delta + (size_t)La * bp * actor_hidden;
    s.heads = s.dh + 16 * bp;
    s.eps = s.heads + 2 * A * bp;
    s.dqda = s.eps + A * bp;
    s.q = s.dqda + 2 * A * bp;
    s.lp = s.q + 2 * bp;
    s.lpart = s.lp + bp;
    fa.s = s; fa.rows = rows; fa.n = batch; fa.S = state_dim; fa.A = A; fa.pitch = pitch; fa.has_critic = has_critic;
    fa.lo = log_std_min; fa.hi = log_std_max; fa.max_action = max_action;
    fa.k0 = (uint32_t)seed; fa.k1 = (uint32_t)(seed >> 32); fa.d0 = (uint32_t)draw; fa.d1 = (uint32_t)(draw >> 32);
    fa.eps_in = eps_in; fa.new_actions = new_actions; fa.log_prob = log_prob; fa.heads = heads; fa.eps_out = eps_out;
    fa.q = has_critic ? q : nullptr; fa.dq_da = has_critic ? dq_da : nullptr;
    ba.s = s; ba.n = batch; ba.A = A; ba.has_critic = has_critic; ba.lo = log_std_min; ba.hi = log_std_max;
    ba.max_action = max_action; ba.target_entropy = target_entropy; ba.log_alpha = log_alpha; ba.weights = weights;
    ba.dheads_in = dheads_in; ba.dheads_out = dheads_out;
    wa.s = s; wa.n = batch; wa.S = state_dim; wa.A = A; wa.pitch = pitch; wa.L = La; wa.has_critic = has_critic;
    wa.rows = rows; wa.log_alpha = log_alpha; wa.actor_loss = actor_loss; wa.alpha_loss = alpha_loss;
    wa.log_alpha_grad = log_alpha_grad; wa.sumsq = sumsq_partials;
    const dim3 grid_a((unsigned)(bp / kSacTile), has_critic ? 2 : 1), grid_b((unsigned)(bp / kSacTile));
    const dim3 grid_c((unsigned)need_partials);
    hipStream_t st = (hipStream_t)stream;
#define PD_ACT_FWD(HA, HC) hipLaunchKernelGGL((k_actor_fwd<HA, HC>), grid_a, dim3(kSacBlock), 0, st, fa)
#define PD_ACT_LAUNCH(HA)                                                                   \
    switch (has_critic ? critic_hidden : 128) {                                             \
        case 128: PD_ACT_FWD(HA, 128); break;                                               \
        case 512: PD_ACT_FWD(HA, 512); break;                                               \
        default: PD_ACT_FWD(HA, 256); break;                                                \
    }                                                                                       \
    hipLaunchKernelGGL(k_actor_bwd<HA>, grid_b, dim3(kSacBlock), 0, st, ba);                \
    hipLaunchKernelGGL(k_actor_wgrad<HA>, grid_c, dim3(kSacBlock), 0, st, wa)
    switch (actor_hidden) {
        case 128: PD_ACT_LAUNCH(128); break;
        case 512: PD_ACT_LAUNCH(512); break;
        default: PD_ACT_LAUNCH(256); break;
    }
#undef PD_ACT_LAUNCH
#undef PD_ACT_FWD
    if (hipGetLastError() != hipSuccess) return set_error(PD_ERR_HIP, "pd_sac_actor_grad: launch failed");
    if (n_partials) *n_partials = need_partials;
    return PD_OK;
}

}  // extern "C"
