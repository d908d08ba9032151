// pdsactd.hip -- the inference-only third of the SAC update on the device: pd_sac_critic, the twin
// critic's forward pass (Critic.forward, sac_pytorch.py:181-221), and pd_sac_td_target, the whole
// torch.no_grad() block of SACPyTorch.update (sac_pytorch.py:439-443) -- actor.sample(next_state),
// critic_target(next_state, next_action), the entropy-regularised minimum and the Bellman backup --
// in one launch each.  No env handle: device pointers, the current HIP device, no host
// synchronisation, nothing read back.
//
// Every MLP here is pd_sac_mlp.h's sac_mlp_tile: 16 rows per 256-thread workgroup, layer 1 on the
// VALU, hidden layers on MFMA, activations in LDS.  A Q net is the actor's stack with the input
// state | action (staged in LDS and handed over as obs_lds) and ONE output (SacQNet: the head stage
// computes A = 1 output instead of 2A), so its sums are the actor's sums in the actor's order.
//
// Grid shapes.
//   pd_sac_critic:    (row tiles, 2): blockIdx.y picks Q1 or Q2.  The two nets share nothing but 16
//                     rows of at most 16 floats, and at B = 256 (16 row tiles) a CU runs one tile of
//                     one net either way: 32 workgroups on 32 CUs take one MLP's time, 16 would take
//                     two.  Nothing joins the two columns, so no workgroup waits for another.
//   pd_sac_td_target: (row tiles): a workgroup runs the actor, samples, then Q1 and Q2 one after
//                     the other for its 16 rows.  The backup needs fminf(q1, q2) of a row, so
//                     splitting the critics over workgroups as above would need either a second
//                     launch or a device-scope join (a counter the last workgroup of a pair waits
//                     on, in memory the library would have to own, since there is no handle) and each
//                     of the pair would run the actor again.  One launch without a join was chosen:
//                     three MLP passes in a row per workgroup, 16 (B = 256) or 32 (B = 512)
//                     workgroups.  The measured times are in DESIGN.md s6.
//
// eps.  Given (eps_in) or drawn here: Philox4x32-10 with key (lo32(seed), hi32(seed)) and counter
// (row, lo32(draw), hi32(draw), kTagTdEps + k / 2), components k = 2m and 2m + 1 from one block by
// gauss_pair's Box-Muller (u1 = 1 - u01(x, y), u2 = u01(z, w), rho = sqrt(-2 log u1), rho cos 2 pi
// u2 and rho sin 2 pi u2, sincos_fd) in binary64, cast to float32.  A draw depends on (seed, draw,
// row, k) only.  The log: gauss_pair reads log_tab's cell table out of an env handle's parameter
// block; this unit has no handle, so it uses pd_log (pd_common.h: fdlibm's e_log.c in plain IEEE
// arithmetic, error below 1 ulp of binary64) and needs no table and no memory of its own.
#include <hip/hip_runtime.h>

#include "../../include/pdenv.h"
#include "pd_common.h"
#include "pd_sac_mlp.h"

namespace {

using namespace pd;

constexpr int kMaxIn = 16;     // state_dim + action_dim of a Q net (sac_mlp_tile's layer 1: K <= 16)
constexpr int kHeadPitch = 16; // a row's heads in LDS: mean at k, log_std at 8 + k (A <= 8)

struct QPair { SacQNet q[2]; };

// state | action of the tile's rows (zeros past n) into sa [16][S + A]
__device__ __forceinline__ void stage_state_action(float* sa, int64_t n, int64_t e0, int S, int A,
                                                   const float* __restrict__ states,
                                                   const float* __restrict__ actions) {
    const int tid = threadIdx.x, D = S + A;
    if (tid < kSacTile * D) {
        const int te = tid / D, c = tid - te * D;
        const int64_t ge = e0 + te;
        sa[tid] = ge < n ? (c < S ? states[ge * S + c] : actions[ge * A + (c - S)]) : 0.f;
    }
}

template <int H>
__global__ __launch_bounds__(kSacBlock) void k_sac_critic(QPair nets, int64_t n, int S, int A,
                                                          const float* __restrict__ states,
                                                          const float* __restrict__ actions, float* __restrict__ q) {
    __shared__ __attribute__((aligned(16))) float hb[sac_mlp_lds_floats<H>()];
    __shared__ float sa[kSacTile * kMaxIn];
    const int64_t e0 = (int64_t)blockIdx.x * kSacTile;
    const int which = blockIdx.y;
    stage_state_action(sa, n, e0, S, A, states, actions);
    __syncthreads();
    sac_mlp_tile<H>(nets.q[which], n, e0, hb, [&](int e, int, float v) {
        const int64_t ge = e0 + e;
        if (ge < n) q[ge * 2 + which] = v;
    }, NoMark{}, sa);
}

// gauss_pair (pd_common.h) with pd_log in place of the handle's log table
__device__ __forceinline__ void gauss_pair_nt(u32x4 r, double& z0, double& z1) {
    const double u1 = 1.0 - u01(r.x, r.y), u2 = u01(r.z, r.w);
    const double rho = sqrt(-2.0 * pd_log(u1));
    double s, c;
    sincos_fd(6.283185307179586 * u2, s, c);
    z0 = rho * c;
    z1 = rho * s;
}

struct TdArgs {
    SacMlp actor;
    QPair critic;
    const float* rows;
    int64_t batch;
    int32_t S, A, width;
    float lo, hi, max_action, gamma;
    const float* log_alpha;
    uint32_t k0, k1, d0, d1;
    const float* eps_in;
    float* target_q;
    float* next_actions;
    float* next_log_prob;
    float* next_q;
    float* heads;
    float* eps_out;
};

template <int HA, int HC>
__global__ __launch_bounds__(kSacBlock) void k_sac_td_target(TdArgs t) {
    constexpr int HM = HA > HC ? HA : HC;
    __shared__ __attribute__((aligned(16))) float hb[sac_mlp_lds_floats<HM>()];
    __shared__ float s_ns[kSacTile * kMaxIn];          // next_state [16][S]: the actor's observations
    __shared__ float s_sa[kSacTile * kMaxIn];          // next_state | next_action [16][S + A]: the critics'
    __shared__ float s_heads[kSacTile * kHeadPitch];
    __shared__ float s_lp[kSacTile * 8];
    __shared__ float s_rd[kSacTile * 2];               // reward, done
    __shared__ float s_q[kSacTile * 2];
    const int tid = threadIdx.x;
    const int S = t.S, A = t.A, D = S + A, W = t.width;
    const int64_t n = t.batch;
    const int64_t e0 = (int64_t)blockIdx.x * kSacTile;
    // ---- the tile's rows, read once: reward | next_state | done (columns S + A .. W - 1; the
    // state and action columns are not this block's); zeros past n
    const int c0 = D, nc = W - D;                        // S + 2 columns
    for (int i = tid; i < kSacTile * nc; i += kSacBlock) {
        const int te = i / nc, c = i - te * nc;
        const int64_t ge = e0 + te;
        const float v = ge < n ? t.rows[ge * W + c0 + c] : 0.f;
        if (c == 0) s_rd[2 * te] = v;
        else if (c == nc - 1) s_rd[2 * te + 1] = v;
        else { s_ns[te * S + (c - 1)] = v; s_sa[te * D + (c - 1)] = v; }
    }
    __syncthreads();
    // ---- 1. heads = Actor.forward(next_state), pd_sac_actor's bits
    sac_mlp_tile<HA>(t.actor, n, e0, hb, [&](int e, int o, float v) {
        s_heads[e * kHeadPitch + (o < A ? o : 8 + (o - A))] = v;
        const int64_t ge = e0 + e;
        if (t.heads && ge < n) t.heads[ge * 2 * A + o] = v;
    }, NoMark{}, s_ns);
    __syncthreads();
    // ---- 2-4. eps, the sampled action and the log-probability's terms: thread (row te, component k)
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
                    const u32x4 r = philox({(uint32_t)ge, t.d0, t.d1, kTagTdEps + (uint32_t)(k >> 1)}, t.k0, t.k1);
                    double z0, z1;
                    gauss_pair_nt(r, z0, z1);
                    ek = (float)((k & 1) ? z1 : z0);
                }
            }
            const float x = m + sd * ek;
            const float a = tanhf(x);
            const float act = a * t.max_action;
            const float d = x - m;
            // Normal.log_prob and the tanh correction (sac_pytorch.py:173-177), torch's order
            const float lp = -(d * d) / (2.f * (sd * sd)) - ls - 0.9189385332046727f - logf(1.f - a * a + 1e-6f);
            s_lp[te * 8 + k] = lp;
            s_sa[te * D + S + k] = act;
            if (ge < n) {
                if (t.eps_out) t.eps_out[ge * A + k] = ek;
                if (t.next_actions) t.next_actions[ge * A + k] = act;
            }
        }
    }
    __syncthreads();
    // ---- 5. the twin target critics on next_state | next_action, pd_sac_critic's bits
    for (int which = 0; which < 2; ++which) {
        sac_mlp_tile<HC>(t.critic.q[which], n, e0, hb, [&](int e, int, float v) { s_q[2 * e + which] = v; },
                         NoMark{}, s_sa);
        __syncthreads();
    }
    // ---- 6. the backup: thread te, row e0 + te
    if (tid < kSacTile && e0 + tid < n) {
        const int64_t ge = e0 + tid;
        float lp = s_lp[tid * 8];
        for (int k = 1; k < A; ++k) lp += s_lp[tid * 8 + k];
        const float alpha = expf(*t.log_alpha);
        const float q1 = s_q[2 * tid], q2 = s_q[2 * tid + 1];
        const float nq = fminf(q1, q2) - alpha * lp;
        t.target_q[ge] = s_rd[2 * tid] + ((1.f - s_rd[2 * tid + 1]) * t.gamma) * nq;
        if (t.next_log_prob) t.next_log_prob[ge] = lp;
        if (t.next_q) { t.next_q[2 * ge] = q1; t.next_q[2 * ge + 1] = q2; }
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

pd_status pd_sac_critic(int64_t n, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t n_hidden_layers,
                        const float* states, const float* actions, const float* const* params_q1,
                        const float* const* params_q2, float* q, void* stream) {
    if (n < 0 || state_dim < 1 || action_dim < 1 || state_dim + (int64_t)action_dim > kMaxIn || n_hidden_layers < 1 ||
        n_hidden_layers > kSacMaxLayers || !params_q1 || !params_q2 || (n > 0 && (!states || !actions || !q)))
        return set_error(PD_ERR_INVALID, "pd_sac_critic: bad arguments");
    if (!hidden_ok(hidden)) return set_error(PD_ERR_UNSUPPORTED, "pd_sac_critic: hidden width 128, 256 or 512 only");
    if (n == 0) return PD_OK;
    QPair nets{};
    const float* const* ps[2] = {params_q1, params_q2};
    for (int w = 0; w < 2; ++w) {
        const pd_status st = fill_qnet(nets.q[w], state_dim + action_dim, hidden, n_hidden_layers, ps[w]);
        if (st == PD_ERR_INVALID) return set_error(st, "pd_sac_critic: null layer parameter");
        if (st != PD_OK) return set_error(st, "pd_sac_critic: parameter not 16-byte aligned");
    }
    const dim3 grid((unsigned)((n + kSacTile - 1) / kSacTile), 2);
    hipStream_t s = (hipStream_t)stream;
    switch (hidden) {
        case 128: hipLaunchKernelGGL(k_sac_critic<128>, grid, dim3(kSacBlock), 0, s, nets, n, state_dim, action_dim, states, actions, q); break;
        case 512: hipLaunchKernelGGL(k_sac_critic<512>, grid, dim3(kSacBlock), 0, s, nets, n, state_dim, action_dim, states, actions, q); break;
        default: hipLaunchKernelGGL(k_sac_critic<256>, grid, dim3(kSacBlock), 0, s, nets, n, state_dim, action_dim, states, actions, q); break;
    }
    if (hipGetLastError() != hipSuccess) return set_error(PD_ERR_HIP, "pd_sac_critic: launch failed");
    return PD_OK;
}

pd_status pd_sac_td_target(int64_t batch, int32_t state_dim, int32_t action_dim, const float* rows, int32_t width,
                           int32_t actor_hidden, int32_t actor_layers, const float* const* actor_params,
                           float log_std_min, float log_std_max, float max_action, int32_t critic_hidden,
                           int32_t critic_layers, const float* const* params_q1, const float* const* params_q2,
                           const float* log_alpha, float gamma, uint64_t seed, uint64_t draw, const float* eps_in,
                           float* target_q, float* next_actions, float* next_log_prob, float* next_q, float* heads,
                           float* eps_out, void* stream) {
    if (batch < 0 || state_dim < 1 || action_dim < 1 || !actor_params || !params_q1 || !params_q2 || !log_alpha ||
        (batch > 0 && (!rows || !target_q)))
        return set_error(PD_ERR_INVALID, "pd_sac_td_target: bad arguments");
    if (width != 2 * (int64_t)state_dim + action_dim + 2)
        return set_error(PD_ERR_INVALID, "pd_sac_td_target: width must be 2 state_dim + action_dim + 2");
    if (state_dim + (int64_t)action_dim > kMaxIn || action_dim > 8 || actor_layers < 1 || actor_layers > kSacMaxLayers ||
        critic_layers < 1 || critic_layers > kSacMaxLayers)
        return set_error(PD_ERR_UNSUPPORTED, "pd_sac_td_target: state_dim + action_dim <= 16, action_dim <= 8, 1 to 8 hidden layers");
    if (!hidden_ok(actor_hidden) || !hidden_ok(critic_hidden))
        return set_error(PD_ERR_UNSUPPORTED, "pd_sac_td_target: hidden width 128, 256 or 512 only");
    TdArgs t{};
    SacMlp& a = t.actor;
    a.S = state_dim; a.L = actor_layers; a.A = action_dim; a.H = actor_hidden; a.obs = nullptr;
    for (int k = 0; k < 2 * (actor_layers + 2); ++k)
        if (!actor_params[k]) return set_error(PD_ERR_INVALID, "pd_sac_td_target: null actor parameter");
    for (int k = 0; k < 2 * (actor_layers + 2); ++k)
        if ((uintptr_t)actor_params[k] % 16 != 0)
            return set_error(PD_ERR_UNSUPPORTED, "pd_sac_td_target: parameter not 16-byte aligned");
    for (int l = 0; l < actor_layers; ++l) { a.w[l] = actor_params[2 * l]; a.b[l] = actor_params[2 * l + 1]; }
    a.wm = actor_params[2 * actor_layers]; a.bm = actor_params[2 * actor_layers + 1];
    a.ws = actor_params[2 * actor_layers + 2]; a.bs = actor_params[2 * actor_layers + 3];
    const float* const* ps[2] = {params_q1, params_q2};
    for (int w = 0; w < 2; ++w) {
        const pd_status st = fill_qnet(t.critic.q[w], state_dim + action_dim, critic_hidden, critic_layers, ps[w]);
        if (st == PD_ERR_INVALID) return set_error(st, "pd_sac_td_target: null critic parameter");
        if (st != PD_OK) return set_error(st, "pd_sac_td_target: parameter not 16-byte aligned");
    }
    if (batch == 0) return PD_OK;
    if ((batch + kSacTile - 1) / kSacTile > 0x7FFFFFFFll)
        return set_error(PD_ERR_UNSUPPORTED, "pd_sac_td_target: batch above 2^35");
    t.rows = rows; t.batch = batch; t.S = state_dim; t.A = action_dim; t.width = width;
    t.lo = log_std_min; t.hi = log_std_max; t.max_action = max_action; t.gamma = gamma; t.log_alpha = log_alpha;
    t.k0 = (uint32_t)seed; t.k1 = (uint32_t)(seed >> 32); t.d0 = (uint32_t)draw; t.d1 = (uint32_t)(draw >> 32);
    t.eps_in = eps_in; t.target_q = target_q; t.next_actions = next_actions; t.next_log_prob = next_log_prob;
    t.next_q = next_q; t.heads = heads; t.eps_out = eps_out;
    const dim3 grid((unsigned)((batch + kSacTile - 1) / kSacTile));
    hipStream_t s = (hipStream_t)stream;
#define PD_TD_LAUNCH(HA, HC) hipLaunchKernelGGL((k_sac_td_target<HA, HC>), grid, dim3(kSacBlock), 0, s, t)
#define PD_TD_CRITIC(HA)                                                      \
    switch (critic_hidden) {                                                  \
        case 128: PD_TD_LAUNCH(HA, 128); break;                               \
        case 512: PD_TD_LAUNCH(HA, 512); break;                               \
        default: PD_TD_LAUNCH(HA, 256); break;                                \
    }
    switch (actor_hidden) {
        case 128: PD_TD_CRITIC(128); break;
        case 512: PD_TD_CRITIC(512); break;
        default: PD_TD_CRITIC(256); break;
    }
#undef PD_TD_CRITIC
#undef PD_TD_LAUNCH
    if (hipGetLastError() != hipSuccess) return set_error(PD_ERR_HIP, "pd_sac_td_target: launch failed");
    return PD_OK;
}

}  // extern "C"
