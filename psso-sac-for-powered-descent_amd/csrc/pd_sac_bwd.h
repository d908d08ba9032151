// pd_sac_bwd.h -- the backward pieces of the SAC update units (pdsacupd.hip, the critic step;
// pdsacact.hip, the actor step): wave_wgrad, one wave's tile of a weight gradient over the batch
// (both units), and sac_bwd_hidden, the hidden layers' backward chain of one 16-row tile on
// pd_sac_mlp.h's workgroup shape (pdsacact.hip's three chains; k_critic_rows keeps the copy of the
// loop it was written with: routed through this function it compiled to other register counts,
// profiles/sac_actor_update_resource_usage.txt).
#pragma once
#include "pd_sac_mlp.h"

namespace pd {

// One wave's tile of dW = A^T . B over the batch: lane (r, q) gives the left operand's column r
// and the right operand's column r of row b0 + q; four rows an instruction, ascending.  acc[i][m]
// = dW[row 4 q + m][column r of tile i]; accb[m] = the left operand's column sums (against ones)
template <int NT, typename FA, typename FB>
__device__ __forceinline__ void wave_wgrad(int64_t bp, bool bias, FA&& fa, FB&& fb, f32x4 (&acc)[NT], f32x4& accb) {
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    accb = f32x4{0.f, 0.f, 0.f, 0.f};
    // U instructions' operands requested together, then the U (NT + 1) MFMAs in row order: the loop
    // is bound by the latency of its loads (a workgroup a CU, nothing else to run meanwhile)
    auto rows = [&](int64_t b0, auto uc) {
        constexpr int U = decltype(uc)::value;
        float av[U], bvv[U][NT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            av[u] = fa(b0 + 4 * u);
#pragma unroll
            for (int i = 0; i < NT; ++i) bvv[u][i] = fb(b0 + 4 * u, i);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int i = 0; i < NT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bvv[u][i], acc[i], 0, 0, 0);
            if (bias) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], 1.f, accb, 0, 0, 0);
        }
    };
    int64_t b0 = 0;
    for (; b0 + 64 <= bp; b0 += 64) rows(b0, std::integral_constant<int, 16>{});
    for (; b0 < bp; b0 += 16) rows(b0, std::integral_constant<int, 4>{});
}

// The hidden layers' backward of one 16-row tile on MFMA: delta_{l-1} = (delta_l . W_l) (h_{l-1} >
// 0) for l = L - 1 .. 1.  dcur [16][H + 4] in LDS holds delta_{L-1} (written before a workgroup
// barrier by the caller), dnxt is the other buffer; the 16 rows are the MFMA's rows, wave w the
// column tiles w, w + 4, ..., NT at a time; k runs over W_l's rows in blocks of 32, lane group q
// taking k = 32 b + 8 q + j as in the forward pass, W_l read with k over its rows, register-staged
// (a wave instruction reads four 64-byte row segments).  pos(l, row, col): h_l[row][col] > 0;
// keep(l, row, col, v): delta_l[row][col] = v as it is produced.  Called by all 256 threads; ends
// behind a barrier; returns the buffer that holds delta_0.
struct NoKeep { __device__ void operator()(int, int, int, float) const {} };
template <int H, typename Pos, typename Keep = NoKeep>
__device__ __forceinline__ float* sac_bwd_hidden(const float* const* w, int L, float* dcur, float* dnxt, Pos&& pos,
                                                 Keep&& keep = Keep{}) {
    constexpr int P = H + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q4 = lane >> 4;
    constexpr int kTiles = H / 64;
    constexpr int NT = kTiles < 2 ? kTiles : 2;
    constexpr int KB = H / 32;
    for (int l = L - 1; l >= 1; --l) {
        const float* W = w[l];
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
                    const float v = pos(l - 1, row, col) ? acc[i][m] : 0.f;
                    dnxt[row * P + col] = v;
                    keep(l - 1, row, col, v);
                }
            }
        }
        __syncthreads();
        float* tmp = dcur; dcur = dnxt; dnxt = tmp;
    }
    return dcur;
}

}  // namespace pd
