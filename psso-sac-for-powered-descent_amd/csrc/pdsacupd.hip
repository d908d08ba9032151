// pdsacupd.hip -- the second third of the SAC update on the device: the critic step of
// SACPyTorch.update (sac_pytorch.py:445-483 and :530-531) -- the twin critic's forward pass, the
// loss, zero_grad() + backward(), clip_grad_norm_, Adam.step and the Polyak loop -- as three
// launches, and the |td| of step 7 (sac_pytorch.py:526).  pdsactd.hip is the first third (the
// no_grad block that gives target_q).  No env handle: device pointers, the current HIP device, no
// host synchronisation, nothing read back, no float atomics: every sum has a fixed order.
//
//   pd_sac_critic_grad   pass a, k_critic_rows, grid (row tiles, 2 nets) as k_sac_critic: the
//                        forward pass on sac_mlp_tile (q is pd_sac_critic's bits), each layer's
//                        post-ReLU tile copied from LDS to scratch at the end of its phase; the
//                        loss gradient of the 16 rows; the backward chain delta_{l-1} = (delta_l .
//                        W_l) * (h_{l-1} > 0) on the 16x16x4 f32 MFMA with the delta tiles in the
//                        LDS the forward pass has left (two buffers of 16 rows), W_l read with k
//                        over its rows, register-staged (a wave instruction reads four 64-byte
//                        row segments); every delta to scratch.
//                        pass b, k_critic_wgrad, grid (output tiles of every layer, 2 nets): a
//                        workgroup owns its tile of dW_l = delta_l^T . h_{l-1} and adds the batch
//                        rows in ascending order on MFMA (four rows an instruction), overwrites the
//                        caller's gradient tensors and leaves the sum of squares of what it wrote
//                        in its slot of sumsq_partials.  The bias gradients are MFMAs against a
//                        column of ones, layer 1 the same code on state | action padded to 16
//                        columns, the head the same code with dq in row 0 of the left operand.
//                        The same launch joins the two nets' |target - q| into td_abs and adds the
//                        row tiles' loss partials.
//   pd_adam_step         pass c, k_adam: one launch over a list of up to 64 tensors, 1 024
//                        elements a workgroup: the clip coefficient from sumsq_partials (every
//                        workgroup adds them itself, in index order), Adam in torch's order of
//                        operations, and the Polyak update of a target tensor on the new value.
//
// Why three launches: dW needs every row's delta (a join over the row tiles), the clip
// coefficient needs every gradient element (a join over pass b's workgroups), and a launch
// boundary is the join that needs no memory of the library's own and no spinning workgroup.
#include <hip/hip_runtime.h>

#include "../../include/pdenv.h"
#include "pd_sac_bwd.h"

namespace {

using namespace pd;

constexpr int kMaxIn = 16;          // state_dim + action_dim (sac_mlp_tile's layer 1: K <= 16)
constexpr int kAdamChunk = 1024;    // elements per workgroup of k_adam

struct QPair { SacQNet q[2]; };
struct QGrad {
    float* w[kSacMaxLayers];
    float* b[kSacMaxLayers];
    float* wm; float* bm;
};

// scratch, in floats, Bp = 16 ceil(batch / 16) rows: act [2][L][Bp][H], delta [2][L][Bp][H],
// dq [2][Bp], td [2][Bp], loss partials [Bp / 16][2]
struct Scratch {
    float* act; float* delta; float* dq; float* td; float* lpart;
};

__host__ __device__ inline int64_t pad16(int64_t b) { return (b + 15) / 16 * 16; }

size_t scratch_floats(int64_t batch, int32_t H, int32_t L) {
    const int64_t bp = pad16(batch);
    return (size_t)(4 * (int64_t)L * H * bp + 4 * bp + bp / 8);
}

// workgroups of pass b per net: layer 1 (4 row tiles of dW each), the hidden layers (a row tile
// by 128 columns each), the head (128 columns each)
__host__ __device__ inline int wg_layer1(int H) { return H / 64; }
__host__ __device__ inline int wg_hidden(int H) { return (H / 16) * (H / 128); }
__host__ __device__ inline int wg_head(int H) { return H / 128; }
__host__ __device__ inline int wg_net(int H, int L) { return wg_layer1(H) + (L - 1) * wg_hidden(H) + wg_head(H); }

struct RowArgs {
    QPair nets;
    Scratch s;
    int64_t n;
    int32_t D, pitch, kind;
    const float* sa;
    const float* target;
    const float* weights;
    const float* dq_in;
    float* q;
    float* dq_out;
};

template <int H>
__global__ __launch_bounds__(kSacBlock) void k_critic_rows(RowArgs a) {
    __shared__ __attribute__((aligned(16))) float hb[sac_mlp_lds_floats<H>()];
    __shared__ float s_sa[kSacTile * kMaxIn];
    __shared__ float s_q[kSacTile], s_dq[kSacTile], s_loss[kSacTile];
    constexpr int P = H + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int which = blockIdx.y;
    const SacQNet& net = a.nets.q[which];
    const int L = net.L, D = a.D;
    const int64_t n = a.n, bp = pad16(n);
    const int64_t e0 = (int64_t)blockIdx.x * kSacTile;
    float* act = a.s.act + (size_t)which * L * bp * H;      // [L][bp][H]
    float* delta = a.s.delta + (size_t)which * L * bp * H;
    // ---- state | action of the tile's rows (zeros past n): the first D floats of each row
    if (tid < kSacTile * D) {
        const int te = tid / D, c = tid - te * D;
        const int64_t ge = e0 + te;
        s_sa[tid] = ge < n ? a.sa[ge * a.pitch + c] : 0.f;
    }
    __syncthreads();
    // ---- forward: pd_sac_critic's code; at the end of phase k < L the layer's post-ReLU tile
    // (sac_mlp_tile's LDS: layer 1 and the even hidden layers in its first buffer, the odd ones in
    // its second) goes to act[k]
    auto keep = [&](int k) {
        if (k >= L) return;
        const float* src = (k & 1) ? hb + kSacTile * P : hb;
        float* dst = act + ((size_t)k * bp + e0) * H;
        for (int i = tid; i < kSacTile * (H / 4); i += kSacBlock) {
            const int row = i / (H / 4), c4 = i - row * (H / 4);
            *(f32x4*)(dst + (size_t)row * H + 4 * c4) = *(const f32x4*)(src + row * P + 4 * c4);
        }
    };
    sac_mlp_tile<H>(net, n, e0, hb, [&](int e, int, float v) {
        s_q[e] = v;
        const int64_t ge = e0 + e;
        if (a.q && ge < n) a.q[ge * 2 + which] = v;
    }, keep, s_sa);
    __syncthreads();
    // ---- the loss gradient of the rows: thread te, row e0 + te
    if (tid < kSacTile) {
        const int64_t ge = e0 + tid;
        float dq = 0.f, lt = 0.f, tdv = 0.f;
        if (ge < n) {
            const float q = s_q[tid];
            if (a.target) {
                const float t = a.target[ge], d = q - t;
                const float w = a.weights ? a.weights[ge] : 1.f;
                const float bf = (float)n;
                tdv = fabsf(t - q);
                if (a.kind == PD_SAC_LOSS_L1) {
                    lt = w * fabsf(d);
                    dq = (w * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f))) / bf;
                } else {
                    lt = w * (d * d);
                    dq = ((2.f * w) * d) / bf;
                }
            }
            if (a.dq_in) dq = a.dq_in[ge * 2 + which];
            if (a.dq_out) a.dq_out[ge * 2 + which] = dq;
        }
        s_dq[tid] = dq;
        s_loss[tid] = lt;
        a.s.dq[which * bp + ge] = dq;
        a.s.td[which * bp + ge] = tdv;
    }
    __syncthreads();
    if (tid == 0) {
        float s = s_loss[0];
        for (int k = 1; k < kSacTile; ++k) s += s_loss[k];
        a.s.lpart[blockIdx.x * 2 + which] = s;
    }
    // ---- the head's backward: delta_{L-1}[b][j] = dq[b] wm[j] (h_{L-1}[b][j] > 0)
    float* dcur = hb;
    float* dnxt = hb + kSacTile * P;
    {
        const float* hl = act + ((size_t)(L - 1) * bp + e0) * H;
        float* dl = delta + ((size_t)(L - 1) * bp + e0) * H;
        for (int i = tid; i < kSacTile * H; i += kSacBlock) {
            const int row = i / H, col = i - row * H;
            const float v = hl[(size_t)row * H + col] > 0.f ? s_dq[row] * net.wm[col] : 0.f;
            dcur[row * P + col] = v;
            dl[(size_t)row * H + col] = v;
        }
    }
    __syncthreads();
    // (this loop and pd_sac_bwd.h's sac_bwd_hidden are the same chain and must be kept in step: routed
    // through that function this kernel compiled to other register counts, so it keeps its copy)
    // ---- the hidden layers' backward on MFMA: delta_{l-1} = (delta_l . W_l) (h_{l-1} > 0); the 16
    // rows are the MFMA's rows, wave w the column tiles w, w + 4, ..., NT at a time; k runs over
    // W_l's rows in blocks of 32, lane group q taking k = 32 b + 8 q + j as in the forward pass
    const int r = lane & 15, q4 = lane >> 4;
    constexpr int kTiles = H / 64;
    constexpr int NT = kTiles < 2 ? kTiles : 2;
    constexpr int KB = H / 32;
    for (int l = L - 1; l >= 1; --l) {
        const float* W = net.w[l];
        const float* hl = act + ((size_t)(l - 1) * bp + e0) * H;
        float* dl = delta + ((size_t)(l - 1) * bp + e0) * H;
#pragma unroll 1
        for (int g = 0; g < kTiles; g += NT) {
            f32x4 acc[NT];
            float bv[2][8][NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            auto fetch = [&](int kb, float (&dst)[8][NT]) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int i = 0; i < NT; ++i)
                        dst[j][i] = W[(size_t)(32 * kb + 8 * q4 + j) * H + 16 * (wave + 4 * (g + i)) + r];
            };
            fetch(0, bv[0]);
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                if (kb + 1 < KB) fetch(kb + 1, bv[(kb + 1) & 1]);
                const float* ap = dcur + r * P + 32 * kb + 8 * q4;
                const f32x4 a0 = *(const f32x4*)ap, a1 = *(const f32x4*)(ap + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < NT; ++i)
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], bv[kb & 1][j][i], acc[i], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < NT; ++i)
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], bv[kb & 1][4 + j][i], acc[i], 0, 0, 0);
            }
            // D[row 4 q + m][col r]
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int col = 16 * (wave + 4 * (g + i)) + r;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int row = 4 * q4 + m;
                    const float v = hl[(size_t)row * H + col] > 0.f ? acc[i][m] : 0.f;
                    dnxt[row * P + col] = v;
                    dl[(size_t)row * H + col] = v;
                }
            }
        }
        __syncthreads();
        float* tmp = dcur; dcur = dnxt; dnxt = tmp;
    }
}

struct WArgs {
    QGrad g[2];
    Scratch s;
    int64_t n;
    int32_t D, pitch, L, kind, per;
    const float* sa;
    float* td_abs;
    float* loss_out;
    float* sumsq;
};

// (wave_wgrad, one wave's tile of dW = A^T . B over the batch: pd_sac_bwd.h, shared with pdsacact.hip)
template <int H>
__global__ __launch_bounds__(kSacBlock) void k_critic_wgrad(WArgs a) {
    __shared__ float s_ss[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q4 = lane >> 4;
    const int which = blockIdx.y, L = a.L, D = a.D;
    const int64_t n = a.n, bp = pad16(n);
    const QGrad& g = a.g[which];
    const float* act = a.s.act + (size_t)which * L * bp * H;
    const float* delta = a.s.delta + (size_t)which * L * bp * H;
    const float* dq = a.s.dq + which * bp;
    int x = blockIdx.x;
    float ss = 0.f;      // the squares of what this lane writes
    f32x4 accb;
    if (x < wg_layer1(H)) {
        // ---- layer 1: dW_1 [H][D] = delta_0^T . (state | action), wave: row tile 4 x + wave
        const int j0 = 16 * (4 * x + wave);
        f32x4 acc[1];
        wave_wgrad<1>(bp, true,
                      [&](int64_t b0) { return delta[(size_t)(b0 + q4) * H + j0 + r]; },
                      [&](int64_t b0, int) { return (r < D && b0 + q4 < n) ? a.sa[(b0 + q4) * a.pitch + r] : 0.f; },
                      acc, accb);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int row = j0 + 4 * q4 + m;
            if (r < D) { g.w[0][(size_t)row * D + r] = acc[0][m]; ss += acc[0][m] * acc[0][m]; }
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
        // ---- the head: dwm [H] = sum_b dq[b] h_{L-1}[b], dbm = sum_b dq[b]: dq in row 0 of the
        // left operand, the other rows zero
        const int kc = x - wg_layer1(H) - (L - 1) * wg_hidden(H);
        const int k0 = 128 * kc + 32 * wave;
        const bool bias = kc == 0 && wave == 0;
        const float* hl = act + (size_t)(L - 1) * bp * H;
        f32x4 acc[2];
        wave_wgrad<2>(bp, bias,
                      [&](int64_t b0) { return r == 0 ? dq[b0 + q4] : 0.f; },
                      [&](int64_t b0, int i) { return hl[(size_t)(b0 + q4) * H + k0 + 16 * i + r]; },
                      acc, accb);
        if (q4 == 0) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                g.wm[k0 + 16 * i + r] = acc[i][0];
                ss += acc[i][0] * acc[i][0];
            }
            if (bias && r == 0) { g.bm[0] = accb[0]; ss += accb[0] * accb[0]; }
        }
    }
    // ---- this workgroup's sum of squares: a fixed tree over the lanes, then the waves in order
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if (lane == 0) s_ss[wave] = ss;
    __syncthreads();
    if (tid == 0 && a.sumsq)
        a.sumsq[which * wg_net(H, L) + blockIdx.x] = ((s_ss[0] + s_ss[1]) + s_ss[2]) + s_ss[3];
    // ---- td_abs = max of the two nets' |target - q| (sac_pytorch.py:526), the rows dealt over
    // the grid; the loss from the row tiles' partials, tile by tile, by one thread
    if (a.td_abs) {
        const int64_t nb = (int64_t)gridDim.x * gridDim.y, me = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        for (int64_t i = me * kSacBlock + tid; i < n; i += nb * kSacBlock)
            a.td_abs[i] = fmaxf(a.s.td[i], a.s.td[bp + i]);
    }
    if (a.loss_out && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
        float s1 = 0.f, s2 = 0.f;
        for (int64_t t = 0; t < bp / 16; ++t) { s1 += a.s.lpart[2 * t]; s2 += a.s.lpart[2 * t + 1]; }
        const float bf = (float)n;
        // (w l1 + w l2).mean() with PER weights, mean(l1) + mean(l2) without
        a.loss_out[0] = a.per ? (s1 + s2) / bf : s1 / bf + s2 / bf;
    }
}

struct AdamArgs {
    float* p[PD_ADAM_MAX_TENSORS];
    float* g[PD_ADAM_MAX_TENSORS];
    float* m[PD_ADAM_MAX_TENSORS];
    float* v[PD_ADAM_MAX_TENSORS];
    float* t[PD_ADAM_MAX_TENSORS];
    int64_t numel[PD_ADAM_MAX_TENSORS];
    uint32_t first[PD_ADAM_MAX_TENSORS + 1];     // the first workgroup of each tensor
    int32_t nt, n_partials, has_targets;
    float step_size, bc2_sqrt, beta2, w1, w2, eps, max_norm, tau, one_minus_tau;
    const float* sumsq;
    float* grad_norm_out;
};

__global__ __launch_bounds__(256) void k_adam(AdamArgs a) {
    const int tid = threadIdx.x;
    // ---- clip_grad_norm_: total = sqrt(sum of the partials in index order), the same in every
    // workgroup and thread
    float coef = 1.f;
    const bool clip = a.max_norm > 0.f;
    if (clip) {
        float s = 0.f;
        for (int i = 0; i < a.n_partials; ++i) s += a.sumsq[i];
        const float total = sqrtf(s);
        const float c = a.max_norm / (total + 1e-6f);
        coef = c < 1.f ? c : 1.f;
        if (blockIdx.x == 0 && tid == 0 && a.grad_norm_out) a.grad_norm_out[0] = total;
    }
    int k = 0;
    while (k + 1 < a.nt && blockIdx.x >= a.first[k + 1]) ++k;
    const int64_t base = (int64_t)(blockIdx.x - a.first[k]) * kAdamChunk;
    const int64_t numel = a.numel[k];
    float* p = a.p[k];
    float* g = a.g[k];
    float* m = a.m[k];
    float* v = a.v[k];
    float* t = a.has_targets ? a.t[k] : nullptr;
#pragma unroll
    for (int u = 0; u < kAdamChunk / 256; ++u) {
        const int64_t i = base + u * 256 + tid;
        if (i < numel) {
            float gi = g[i];
            if (clip) { gi = gi * coef; g[i] = gi; }
            // Adam.step, torch's order: exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2)
            // .addcmul_(grad, grad, value=1 - beta2); denom = exp_avg_sq.sqrt() / sqrt(bc2) + eps;
            // param.addcdiv_(exp_avg, denom, value=-step_size)
            float mi = m[i], vi = v[i];
            mi = mi + a.w1 * (gi - mi);
            vi = vi * a.beta2;
            vi = vi + (a.w2 * gi) * gi;
            const float denom = sqrtf(vi) / a.bc2_sqrt + a.eps;
            const float pi = p[i] + (-a.step_size) * (mi / denom);
            m[i] = mi; v[i] = vi; p[i] = pi;
            // Polyak on the new value: (1 - tau) * t + tau * p
            if (t) t[i] = a.one_minus_tau * t[i] + a.tau * pi;
        }
    }
}

bool hidden_ok(int32_t h) { return h == 128 || h == 256 || h == 512; }

}  // namespace

namespace pd {
pd_status set_error(pd_status s, const char* m);   // pdenv.hip: the pd_last_error() message
}

extern "C" {

size_t pd_sac_critic_grad_scratch_bytes(int64_t batch, int32_t hidden, int32_t n_hidden_layers) {
    if (batch <= 0 || hidden <= 0 || n_hidden_layers <= 0) return 0;
    return 4 * scratch_floats(batch, hidden, n_hidden_layers);
}

pd_status pd_sac_critic_grad(int64_t batch, int32_t state_dim, int32_t action_dim, int32_t hidden,
                             int32_t n_hidden_layers, const float* sa, int32_t pitch, const float* target_q,
                             const float* weights, int32_t loss_kind, const float* dq_in,
                             const float* const* params_q1, const float* const* params_q2, float* const* grads_q1,
                             float* const* grads_q2, float* q, float* td_abs, float* dq_out, float* loss_out,
                             float* sumsq_partials, int32_t* n_partials, void* scratch, size_t scratch_bytes,
                             void* stream) {
    const int64_t D = (int64_t)state_dim + action_dim;
    const int32_t L = n_hidden_layers;
    if (batch < 0 || state_dim < 1 || action_dim < 1 || D > kMaxIn || L < 1 || L > kSacMaxLayers || !params_q1 ||
        !params_q2 || !grads_q1 || !grads_q2)
        return set_error(PD_ERR_INVALID, "pd_sac_critic_grad: bad arguments");
    if (loss_kind != PD_SAC_LOSS_L2 && loss_kind != PD_SAC_LOSS_L1)
        return set_error(PD_ERR_INVALID, "pd_sac_critic_grad: unknown loss kind");
    if (pitch < D) return set_error(PD_ERR_INVALID, "pd_sac_critic_grad: pitch below state_dim + action_dim");
    if (batch > 0 && (!sa || (!target_q && (!dq_in || td_abs || loss_out))))
        return set_error(PD_ERR_INVALID, "pd_sac_critic_grad: null sa, or no target_q (required unless dq_in is "
                                         "given and neither td_abs nor loss_out is asked for)");
    if (sumsq_partials && !n_partials)
        return set_error(PD_ERR_INVALID, "pd_sac_critic_grad: sumsq_partials without n_partials");
    if (!hidden_ok(hidden)) return set_error(PD_ERR_UNSUPPORTED, "pd_sac_critic_grad: hidden width 128, 256 or 512 only");
    const int32_t need_partials = 2 * wg_net(hidden, L);
    if (sumsq_partials && *n_partials < need_partials)
        return set_error(PD_ERR_INVALID, "pd_sac_critic_grad: sumsq_partials shorter than 2 (H / 64 + (L - 1) (H / 16) "
                                         "(H / 128) + H / 128)");
    RowArgs ra{};
    WArgs wa{};
    const float* const* ps[2] = {params_q1, params_q2};
    float* const* gs[2] = {grads_q1, grads_q2};
    for (int w = 0; w < 2; ++w) {
        SacQNet& net = ra.nets.q[w];
        net.S = (int32_t)D; net.L = L; net.A = 1; net.H = hidden; net.obs = nullptr;
        for (int k = 0; k < 2 * (L + 1); ++k)
            if (!ps[w][k] || !gs[w][k]) return set_error(PD_ERR_INVALID, "pd_sac_critic_grad: null layer parameter or gradient");
        for (int k = 0; k < 2 * (L + 1); ++k)
            if ((uintptr_t)ps[w][k] % 16 != 0 || (uintptr_t)gs[w][k] % 16 != 0)
                return set_error(PD_ERR_UNSUPPORTED, "pd_sac_critic_grad: parameter or gradient not 16-byte aligned");
        for (int l = 0; l < L; ++l) {
            net.w[l] = ps[w][2 * l]; net.b[l] = ps[w][2 * l + 1];
            wa.g[w].w[l] = gs[w][2 * l]; wa.g[w].b[l] = gs[w][2 * l + 1];
        }
        net.wm = ps[w][2 * L]; net.bm = ps[w][2 * L + 1];
        net.ws = net.wm; net.bs = net.bm;      // (never read: one head)
        wa.g[w].wm = gs[w][2 * L]; wa.g[w].bm = gs[w][2 * L + 1];
    }
    if (batch == 0) {
        if (n_partials) *n_partials = 0;
        return PD_OK;
    }
    if ((batch + kSacTile - 1) / kSacTile > 0x7FFFFFFFll)
        return set_error(PD_ERR_UNSUPPORTED, "pd_sac_critic_grad: batch above 2^35");
    const size_t need = 4 * scratch_floats(batch, hidden, L);
    if (!scratch || scratch_bytes < need || (uintptr_t)scratch % 16 != 0)
        return set_error(PD_ERR_INVALID, "pd_sac_critic_grad: scratch missing, misaligned or shorter than "
                                         "pd_sac_critic_grad_scratch_bytes");
    const int64_t bp = pad16(batch);
    Scratch s;
    s.act = (float*)scratch;
    s.delta = s.act + (size_t)2 * L * bp * hidden;
    s.dq = s.delta + (size_t)2 * L * bp * hidden;
    s.td = s.dq + 2 * bp;
    s.lpart = s.td + 2 * bp;
    ra.s = s; ra.n = batch; ra.D = (int32_t)D; ra.pitch = pitch; ra.kind = loss_kind; ra.sa = sa; ra.target = target_q;
    ra.weights = weights; ra.dq_in = dq_in; ra.q = q; ra.dq_out = dq_out;
    wa.s = s; wa.n = batch; wa.D = (int32_t)D; wa.pitch = pitch; wa.L = L; wa.kind = loss_kind; wa.per = weights != nullptr;
    wa.sa = sa; wa.td_abs = td_abs; wa.loss_out = loss_out; wa.sumsq = sumsq_partials;
    const dim3 grid_a((unsigned)(bp / kSacTile), 2), grid_b((unsigned)wg_net(hidden, L), 2);
    hipStream_t st = (hipStream_t)stream;
#define PD_UPD_LAUNCH(HH)                                                                   \
    hipLaunchKernelGGL(k_critic_rows<HH>, grid_a, dim3(kSacBlock), 0, st, ra);              \
    hipLaunchKernelGGL(k_critic_wgrad<HH>, grid_b, dim3(kSacBlock), 0, st, wa)
    switch (hidden) {
        case 128: PD_UPD_LAUNCH(128); break;
        case 512: PD_UPD_LAUNCH(512); break;
        default: PD_UPD_LAUNCH(256); break;
    }
#undef PD_UPD_LAUNCH
    if (hipGetLastError() != hipSuccess) return set_error(PD_ERR_HIP, "pd_sac_critic_grad: launch failed");
    if (n_partials) *n_partials = need_partials;
    return PD_OK;
}

pd_status pd_adam_step(int32_t n_tensors, float* const* params, float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, const int64_t* numel, float* const* targets, double step_size,
                       double bc2_sqrt, double beta1, double beta2, double eps, double max_norm,
                       const float* sumsq_partials, int32_t n_partials, float* grad_norm_out, double tau, void* stream) {
    if (n_tensors < 0 || n_tensors > PD_ADAM_MAX_TENSORS)
        return set_error(PD_ERR_INVALID, "pd_adam_step: n_tensors outside 0 .. PD_ADAM_MAX_TENSORS");
    if (n_tensors > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !numel))
        return set_error(PD_ERR_INVALID, "pd_adam_step: null tensor list");
    if (max_norm > 0 && (!sumsq_partials || n_partials < 1))
        return set_error(PD_ERR_INVALID, "pd_adam_step: clipping needs sumsq_partials");
    AdamArgs a{};
    uint64_t wgs = 0;
    int nt = 0;
    for (int k = 0; k < n_tensors; ++k) {
        if (numel[k] < 0) return set_error(PD_ERR_INVALID, "pd_adam_step: negative numel");
        if (numel[k] == 0) continue;
        if (!params[k] || !grads[k] || !exp_avg[k] || !exp_avg_sq[k] || (targets && !targets[k]))
            return set_error(PD_ERR_INVALID, "pd_adam_step: null tensor");
        a.p[nt] = params[k]; a.g[nt] = grads[k]; a.m[nt] = exp_avg[k]; a.v[nt] = exp_avg_sq[k];
        a.t[nt] = targets ? targets[k] : nullptr;
        a.numel[nt] = numel[k];
        a.first[nt] = (uint32_t)wgs;
        wgs += (uint64_t)((numel[k] + kAdamChunk - 1) / kAdamChunk);
        if (wgs > 0x7FFFFFFFull) return set_error(PD_ERR_UNSUPPORTED, "pd_adam_step: more than 2^41 elements");
        ++nt;
    }
    if (nt == 0) return PD_OK;
    a.first[nt] = (uint32_t)wgs;
    a.nt = nt; a.n_partials = max_norm > 0 ? n_partials : 0; a.has_targets = targets != nullptr;
    a.step_size = (float)step_size; a.bc2_sqrt = (float)bc2_sqrt; a.beta2 = (float)beta2;
    a.w1 = (float)(1.0 - beta1); a.w2 = (float)(1.0 - beta2); a.eps = (float)eps;
    a.max_norm = max_norm > 0 ? (float)max_norm : 0.f;
    a.tau = (float)tau; a.one_minus_tau = (float)(1.0 - tau);
    a.sumsq = sumsq_partials; a.grad_norm_out = grad_norm_out;
    hipLaunchKernelGGL(k_adam, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, a);
    if (hipGetLastError() != hipSuccess) return set_error(PD_ERR_HIP, "pd_adam_step: launch failed");
    return PD_OK;
}

}  // extern "C"
