// pdenv.hip -- the handle and C ABI of libpdenv.so (MI355X / gfx950), plus its small kernels.
//
// The step kernel itself is k_step (pd_step_impl.h), instantiated in the kstep.hip translation
// units, and the parameter block and neighbourhood tables are computed on the host by
// pd_tables.hip (build_host_tables); this unit uploads them, owns the per-env SoA buffers in HBM,
// and launches.  See DESIGN.md for the roofline of each kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pdenv.h"
#include "pd_envdev.h"
#include "pd_tables.h"

using namespace pd;

namespace pd {
// the thread-local message behind pd_last_error(), shared by every source of the library
thread_local std::string g_err;
pd_status set_error(pd_status s, const char* m) { g_err = m; return s; }
}  // namespace pd

namespace {

pd_status fail(pd_status s, const std::string& m) { g_err = m; return s; }

#define PD_HIP(expr)                                                                   \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail(PD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ---------------------------------------------------------------- per-env kernels
// The register state of one env written to its SoA slot (k_reset; the step kernel stores its
// own).  reset_cache: start the aero caches at the handle's initial keys.
template <typename R>
__device__ void store_env(const StepArgs<R>& a, DP<R>& P, uint32_t ui, const EnvRegs<R>& e, bool reset_cache) {
    const int64_t N = a.n;
#pragma unroll
    for (int k = 0; k < 11; ++k) ev(a.b.st + (k) * N, ui) = e.s[k];
    ev(a.b.vprev, ui) = e.vprev;
    ev(a.b.ghead, ui) = (uint8_t)e.ghead; ev(a.b.glen, ui) = (uint8_t)e.glen;
    ev(a.b.act, ui) = e.act0; ev(a.b.act + N, ui) = e.act1; ev(a.b.act + (2) * N, ui) = e.act2;
    ev(a.b.tid, ui) = (int8_t)e.tid;
    ev(a.b.epi, ui) = e.ep; ev(a.b.tstep, ui) = e.ts;
    ev(a.b.fin, ui) = 0;
    ev(a.b.wind, ui) = e.fu0; ev(a.b.wind + N, ui) = e.fu1; ev(a.b.wind + (2) * N, ui) = e.fv0; ev(a.b.wind + (3) * N, ui) = e.fv1;
    ev(a.b.wind + (4) * N, ui) = e.sgu; ev(a.b.wind + (5) * N, ui) = e.sgv;
    ev(a.b.wprof, ui) = (uint8_t)e.prof;
    if (reset_cache) {   // any valid 50-set is a correct start for the swap search
        ev(a.b.key, ui) = P.init_key_cd; ev(a.b.key + N, ui) = P.init_key_cl;
        ev(a.b.slot, ui) = -1; ev(a.b.slot + N, ui) = -1;
    }
}

// rocket_environment_pre_wrap.reset (base_environment.py:80-97) of every (masked) env
template <typename R>
__global__ __launch_bounds__(kBlock) void k_reset(StepArgs<R> a, const uint8_t* mask) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    if (mask && !mask[i]) return;
    DP<R>& P = *params<R>(a.P);
    const uint32_t ui = (uint32_t)i;
    EnvRegs<R> e;
    reset_values<R>(P, a, a.env_offset + (uint64_t)i, ev(a.b.epi, ui) + 1u,
                    (const double*)(uint64_t)&P.logtab.invc[0], (const double*)(uint64_t)&P.logtab.logc[0], e);
    store_env<R>(a, P, ui, e, true);
}

// Insert the neighbourhoods solved on device during the last launch (single thread; the only
// writer of the tables, stream-ordered between launches, so readers never race it).  The step
// launches insert their own (their last workgroup, k_step); this serves the policy rollouts and
// pd_flush_misses.
template <typename R>
__global__ void k_insert(Pending pend, unsigned long long* keys_cd, R* pay_cd, int lc_cd,
                         unsigned long long* keys_cl, R* pay_cl, int lc_cl) {
    if (threadIdx.x == 0) insert_pending<R>(pend.count, pend.keys, pend.pay, pend.stats, keys_cd, pay_cd, lc_cd, keys_cl, pay_cl, lc_cl);
}

template <typename R>
__global__ __launch_bounds__(kBlock) void k_observe(StepArgs<R> a, int obs_kind) {
    DP<R>& P = *params<R>(a.P);
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t N = a.n;
    if (i >= N) return;
    R s[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) s[k] = a.b.st[k * N + i];
    obs_write<R>(P, obs_kind, s, a.obs, (uint32_t)i);
}

// endo_atmospheric_model (atmosphere_dynamics.py:5-27) at n altitudes: out [3][n] = rho, p, a
template <typename R>
__global__ __launch_bounds__(kBlock) void k_atmosphere(StepArgs<R> a, const R* alt, R* out, int64_t n) {
    __shared__ R isa[9 * kIsaCols];
    DP<R>& P = *params<R>(a.P);
    if (threadIdx.x < 9) {
        const int k = threadIdx.x;
        R* r = isa + k * kIsaCols;
        r[0] = P.isa_Hb[k]; r[1] = P.isa_Tb[k]; r[2] = P.isa_beta[k]; r[3] = P.isa_pb[k];
        r[4] = P.isa_bt[k]; r[5] = P.isa_ex[k]; r[6] = P.isa_iso[k]; r[7] = R(0);
    }
    for (int t = threadIdx.x; t < 2 * kLogCellsD; t += kBlock) {
        s_logtab[t] = P.logtab_d.cell[t];
    }
    __syncthreads();
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    R rho, pr, as;
    atmosphere<R>(P, isa, alt[i], rho, pr, as);
    out[i] = rho; out[n + i] = pr; out[2 * n + i] = as;
}

template <typename R>
__global__ __launch_bounds__(kBlock) void k_set_sigmas(StepArgs<R> a, const double* sig) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    a.b.wind[4 * a.n + i] = (R)sig[i];
    a.b.wind[5 * a.n + i] = (R)sig[a.n + i];
}

// ---------------------------------------------------------------- host side
// The device copy of a table's cell pieces: one per device and process, shared read-only by the
// handles (never freed; ~0.2 GB of the 288 GB)
template <typename R>
pd_status cell_pieces_device(const CellPieces& cp, const R** rec, const int** sub, const uint32_t** fine) {
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, std::array<void*, 3>> m;
    const bool f32 = sizeof(R) == 4;
    const auto& rv = f32 ? (const void*)cp.rec32.data() : (const void*)cp.rec.data();
    const size_t rbytes = f32 ? cp.rec32.size() * 4 : cp.rec.size() * 8;
    const std::vector<int>& sp = f32 ? cp.sub_piece32 : cp.sub_piece;
    const std::vector<uint32_t>& fn = f32 ? cp.fine32 : cp.fine;
    int dev = 0;
    PD_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    auto k = std::make_pair((const void*)(f32 ? (const void*)&cp.rec32 : (const void*)&cp.rec), dev);
    auto it = m.find(k);
    if (it == m.end()) {
        std::array<void*, 3> d{};
        const void* src[3] = {rv, sp.data(), fn.data()};
        const size_t nb[3] = {rbytes, sp.size() * 4, fn.size() * 4};
        for (int q = 0; q < 3; ++q) {
            PD_HIP(hipMalloc(&d[q], std::max<size_t>(nb[q], 8)));
            if (nb[q]) PD_HIP(hipMemcpy(d[q], src[q], nb[q], hipMemcpyHostToDevice));
        }
        it = m.emplace(k, d).first;
    }
    *rec = (const R*)it->second[0];
    *sub = (const int*)it->second[1];
    *fine = (const uint32_t*)it->second[2];
    return PD_OK;
}

}  // namespace

// ---------------------------------------------------------------- the handle
struct pd_env {
    pd_config cfg{};
    int device = 0;
    int obs_dim = 2, act_dim = 1;
    size_t rsize = 8;
    void* dparams = nullptr;
    std::vector<void*> allocs;
    // per-env buffers (typed views in the precision of the handle)
    void* st = nullptr; void* vprev = nullptr; void* gwin = nullptr; void* act = nullptr; void* wind = nullptr;
    uint8_t *ghead = nullptr, *glen = nullptr, *wprof = nullptr;
    unsigned long long* key = nullptr; int* slot = nullptr;
    int8_t* tid = nullptr; uint32_t *epi = nullptr, *tstep = nullptr;
    uint8_t* fin = nullptr;
    int32_t* live[2] = {nullptr, nullptr};   // policy rollouts: compacted live-env lists
    uint32_t* live_cnt = nullptr;            // [3] their lengths (triple-buffered)
    uint32_t* host_cnt = nullptr;            // [2] pinned host copies of checked lengths
    hipEvent_t cnt_ev[2] = {nullptr, nullptr};
    Pending pend{};
    unsigned long long *keys_cd = nullptr, *keys_cl = nullptr;
    void *pay_cd = nullptr, *pay_cl = nullptr;
    int logcap_cd = 0, logcap_cl = 0;
    int64_t entries_cd = 0, entries_cl = 0;
    int lpe = 2;   // lanes per env of the step kernel
    int obs_kind = 0;   // obs_write layout of the handle's observation
    int count_work = 0; // workload counters on (pd_count_work)
    float* sac_heads = nullptr;   // pd_step_sac_fused's two-launch path: the actor heads [N][2A]
    void* roll_ret = nullptr;     // pd_rollout_sac without `ret`: the returns carried between its launches [N]
    float* pol_w4 = nullptr;      // policy rollouts: the actor parameters in chunks of four ([P/4][N][4])
    float* pol_wc = nullptr;      // policy rollouts' list launches: the live envs' actor parameters
    pd_tuning tune{128, 64, 2, -1, 0.0, -1, 0, -1, 0};   // launch tuning (pd_set_tuning)
};

namespace {
int act_dim_of(int phase) {
    return phase == PD_PHASE_LANDING_BURN ? 4 : ((phase == PD_PHASE_SUBSONIC || phase == PD_PHASE_SUPERSONIC) ? 2 : 1);
}
}  // namespace

namespace {

pd_status dalloc(pd_env* e, void** p, size_t bytes) {
    if (bytes == 0) bytes = 8;
    PD_HIP(hipMalloc(p, bytes));
    e->allocs.push_back(*p);
    return PD_OK;
}

template <typename R> StepArgs<R> make_args(pd_env* e) {
    StepArgs<R> a{};
    a.P = (uint64_t)e->dparams;
    a.b.st = (R*)e->st; a.b.vprev = (R*)e->vprev; a.b.gwin = (R*)e->gwin; a.b.ghead = e->ghead; a.b.glen = e->glen;
    a.b.act = (R*)e->act; a.b.wind = (R*)e->wind; a.b.wprof = e->wprof; a.b.key = e->key; a.b.slot = e->slot;
    a.b.tid = e->tid; a.b.epi = e->epi; a.b.tstep = e->tstep; a.b.fin = e->fin;
    a.pend = e->pend;
    a.n = e->cfg.n_envs;
    a.env_offset = e->cfg.env_offset;
    a.seed_lo = (uint32_t)e->cfg.seed; a.seed_hi = (uint32_t)(e->cfg.seed >> 32);
    a.act_f64 = e->cfg.action_f64;
    a.auto_reset = e->cfg.auto_reset;
    a.stochastic = e->cfg.stochastic_wind;
    a.fixed_prof = e->cfg.wind_percentile >= 50 ? e->cfg.wind_percentile - 50 : -1;
    a.use_tilt = e->cfg.tilt_sigma_rad > 0.0;
    a.tilt_sigma = e->cfg.tilt_sigma_rad;
    a.dt_aux = e->cfg.dt > 0.0 ? e->cfg.dt : 0.1;
    a.rtd_none = e->cfg.rtd == PD_RTD_NONE;
    a.n_fused = 1;
    a.count_work = (e->count_work ? kArgCount : 0) | ((e->cfg.table_flags & PD_TABLES_NO_CARRY) ? kArgNoCarry : 0) |
                   ((e->cfg.table_flags & PD_TABLES_NO_PACE) ? kArgNoPace : 0);
    return a;
}

// f(R{}) with R the handle's real type: the one place a precision becomes a template argument
template <typename F> auto with_real(bool f64, F&& f) {
    if (f64) return f(double{});
    return f(float{});
}
template <typename F> auto with_real(const pd_env* e, F&& f) { return with_real(e->rsize == 8, f); }

pd_status validate(const pd_params* p, const pd_config* c) {
    if (!p || !c) return fail(PD_ERR_INVALID, "null params/config");
    // per-lane byte offsets in k_step are 32-bit (largest per-env row: noise, 64 B)
    if (c->n_envs <= 0 || c->n_envs > (int64_t)1 << 25) return fail(PD_ERR_INVALID, "n_envs out of range (1 .. 2^25 per handle)");
    if (c->phase < 0 || c->phase > PD_PHASE_LANDING_BURN_ACS) return fail(PD_ERR_INVALID, "bad phase");
    if (c->rtd != PD_RTD_RL && c->rtd != PD_RTD_PSO && c->rtd != PD_RTD_NONE) return fail(PD_ERR_INVALID, "bad rtd");
    if (c->phase == PD_PHASE_LANDING_BURN_ACS)
        return fail(PD_ERR_UNSUPPORTED, "landing_burn_ACS: the reference raises TypeError at its first step "
                                        "(rockets_physics.py:867-891 passes ACS arguments to the gimballed decomposer; "
                                        "base_environment.py:126-130 passes two prevs to a three-prev lambda)");
    if (c->rtd == PD_RTD_RL && c->phase == PD_PHASE_FLIP_OVER)
        return fail(PD_ERR_UNSUPPORTED, "flip_over_boostbackburn with rtd RL: the reference raises TypeError at its first "
                                        "step (rtd_rl.py:134 truncated_func(state) called with three arguments, "
                                        "base_environment.py:150); use PD_RTD_NONE for physics stepping");
    if (c->rtd == PD_RTD_PSO && c->phase > PD_PHASE_LANDING_BURN)
        return fail(PD_ERR_UNSUPPORTED, "rtd PSO exists for the two landing burns only: the other rtd_pso functions take "
                                        "(state) / (state, done, truncated) and raise TypeError when the env calls them "
                                        "(rtd_pso.py:38,63,107,120,141,157 vs base_environment.py:150-152)");
    if (c->dt < 0.0) return fail(PD_ERR_INVALID, "dt must be >= 0");
    if (c->rtd == PD_RTD_RL && (c->phase == PD_PHASE_LANDING_BURN || c->phase == PD_PHASE_PCONTROL) &&
        (c->trajectory_length < 1 || !(c->discount_factor > 0.0 && c->discount_factor < 1.0)))
        return fail(PD_ERR_INVALID, "this RL reward needs discount_factor in (0, 1) and trajectory_length >= 1");
    if (c->phase == PD_PHASE_SUBSONIC || c->phase == PD_PHASE_SUPERSONIC) {
        if (!p->ref_y || !p->ref_x || !p->ref_vx || !p->ref_vy || p->n_ref < 2)
            return fail(PD_ERR_INVALID, "ascent phases need the reference trajectory (ref_y/x/vx/vy, n_ref >= 2)");
    }
    if (c->precision != PD_F64 && c->precision != PD_F32) return fail(PD_ERR_INVALID, "bad precision");
    if (c->integrator != PD_INTEG_REFERENCE && c->integrator != PD_INTEG_RK4) return fail(PD_ERR_INVALID, "bad integrator");
    if (c->table_flags & ~(PD_TABLES_NO_CELL_PIECES | PD_TABLES_NO_FINE_INDEX | PD_TABLES_EXACT_ATMOSPHERE | PD_TABLES_VERBOSE |
                           PD_TABLES_NO_CARRY | PD_TABLES_NO_ATM_LDS | PD_TABLES_NO_PACE))
        return fail(PD_ERR_INVALID, "unknown table_flags bits");
    if (c->integrator == PD_INTEG_RK4 && (c->phase != PD_PHASE_PURE_THROTTLE || c->enable_wind))
        return fail(PD_ERR_UNSUPPORTED, "the RK4 integrator (non-parity, BASELINE c2) exists for "
                                        "landing_burn_pure_throttle without wind only");
    // the neighbourhood payloads carry each pair slot's column AoA as a byte (pd_common.h)
    for (const pd_aero_table* t : {&p->cd, &p->cl})
        for (int k = 0; k < t->n_cols; ++k)
            if (!(t->col_aoa[k] >= 0.0 && t->col_aoa[k] <= 255.0 && t->col_aoa[k] == (double)(int)t->col_aoa[k]))
                return fail(PD_ERR_INVALID, "aero table column AoAs must be integers in [0, 255]");
    if (c->action_f64 && c->precision != PD_F64) return fail(PD_ERR_INVALID, "f64 actions need PD_F64");
    if (c->enable_wind && !(c->wind_percentile == -1 || (c->wind_percentile >= 50 && c->wind_percentile <= 99)))
        return fail(PD_ERR_INVALID, "wind_percentile must be 50..99 or -1");
    const pd_aero_table* ts[2] = {&p->cd, &p->cl};
    for (auto t : ts) {
        if (t->n_cols != kCols || t->n_pts < kNbr || t->n_pts > PD_MAX_PTS) return fail(PD_ERR_INVALID, "aero table shape");
        int s = 0;
        for (int k = 0; k < kCols; ++k) {
            if (t->col_start[k] != s || t->col_len[k] < 1 || t->col_len[k] >= (1 << kKeyLoBits))
                return fail(PD_ERR_INVALID, "aero column layout");
            s += t->col_len[k];
        }
        if (s != t->n_pts) return fail(PD_ERR_INVALID, "aero column count");
    }
    if (p->ca_n < 2 || p->ca_n > PD_MAX_TAB || p->cn_n < 2 || p->cn_n > PD_MAX_TAB) return fail(PD_ERR_INVALID, "grid fin tables");
    for (int w = 0; w < PD_N_WIND_PROFILES; ++w)
        if (c->enable_wind && (p->wind_n[w] < 1 || p->wind_n[w] > PD_MAX_WIND)) return fail(PD_ERR_INVALID, "wind profile");
    return PD_OK;
}

// One uploaded array: n elements allocated on the handle (pd_destroy frees them), copied from
// the host if there are any; *dev is the typed device pointer
template <typename T, typename P> pd_status upload(pd_env* e, const T* src, size_t n, P** dev) {
    void* d;
    pd_status st = dalloc(e, &d, n * sizeof(T));
    if (st != PD_OK) return st;
    if (n) PD_HIP(hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice));
    *dev = (P*)d;
    return PD_OK;
}
template <typename T, typename P> pd_status upload(pd_env* e, const std::vector<T>& v, P** dev) {
    return upload(e, v.data(), v.size(), dev);
}

// build (pd_tables.hip: every table on the host) -> upload -> per-env buffers -> first reset
template <typename R> pd_status create_impl(const pd_params* p, const pd_config* c, pd_env* e) {
    const int64_t N = c->n_envs;
    HostTables<R> H;
    pd_status st;
    if ((st = build_host_tables<R>(p, c, H)) != PD_OK) return st;
    DevParams<R>& D = H.D;
    if ((st = upload(e, H.tay, &D.tay))) return st;
    if (!H.atm.empty() && (st = upload(e, H.atm, &D.atm_tab))) return st;
    // the cell pieces and the fine index (PD_TABLES_NO_FINE_INDEX: cell and sub-cell records only)
    for (int tb = 0; tb < 2; ++tb) {
        const CellPieces* cp = H.grid[tb].pieces;
        if (cp && (st = cell_pieces_device<R>(*cp, &D.cell_pc[tb], &D.sub_piece[tb], &D.fine[tb])) != PD_OK) return st;
        if (c->table_flags & PD_TABLES_NO_FINE_INDEX) D.fine[tb] = nullptr;
    }
    for (int tb = 0; tb < 2; ++tb) {
        const auto& G = H.grid[tb];
        if ((st = upload(e, G.key, &D.grid_key[tb])) || (st = upload(e, G.slot, &D.grid_slot[tb])) ||
            (st = upload(e, G.sub_key, &D.sub_key[tb])) || (st = upload(e, G.sub_slot, &D.sub_slot[tb])) ||
            (st = upload(e, G.bis, &D.sub_bis[tb])))
            return st;
    }
    e->logcap_cd = H.cd.logcap; e->logcap_cl = H.cl.logcap;
    e->entries_cd = H.cd.entries; e->entries_cl = H.cl.entries;
    if ((st = upload(e, H.cd.keys, &e->keys_cd)) || (st = upload(e, H.cd.pay, &e->pay_cd)) ||
        (st = upload(e, H.cl.keys, &e->keys_cl)) || (st = upload(e, H.cl.pay, &e->pay_cl)))
        return st;
    D.keys_cd = e->keys_cd; D.keys_cl = e->keys_cl; D.pay_cd = (const R*)e->pay_cd; D.pay_cl = (const R*)e->pay_cl;
    if (c->phase == PD_PHASE_SUBSONIC || c->phase == PD_PHASE_SUPERSONIC) {
        // ascent reference trajectory, in the handle's precision (binary-searched per env-step)
        const double* src[4] = {p->ref_y, p->ref_x, p->ref_vx, p->ref_vy};
        const R** dst[4] = {&D.ref_y, &D.ref_x, &D.ref_vx, &D.ref_vy};
        std::vector<R> buf((size_t)p->n_ref);
        for (int k = 0; k < 4; ++k) {
            for (int32_t r = 0; r < p->n_ref; ++r) buf[r] = (R)src[k][r];
            if ((st = upload(e, buf, dst[k]))) return st;
        }
    }
    {
        // the step kernels' LDS tables as one image (pd_step.h StepStatic), copied by their prologue;
        // binary64 wind handles: the BIG image (the 512-thread kernels', of which the other kernels
        // copy the leading StepStatic<R, true>)
        constexpr bool kBigImg = sizeof(R) == 8;
        std::vector<uint8_t> h(c->enable_wind ? sizeof(StepStatic<R, true, kBigImg>) : sizeof(StepStatic<R, false>));
        if (c->enable_wind) {
            if constexpr (kBigImg) fill_step_static_big<R, true>(D, H.atl.data(), H.atl.size(), *(StepStatic<R, true, true>*)h.data());
            else fill_step_static<R, true>(D, *(StepStatic<R, true>*)h.data());
        }
        else fill_step_static<R, false>(D, *(StepStatic<R, false>*)h.data());
        if ((st = upload(e, h, &D.stage_img))) return st;
    }
    if ((st = upload(e, &D, 1, &e->dparams))) return st;
    size_t R_ = sizeof(R);
    if ((st = dalloc(e, &e->st, 11 * N * R_)) || (st = dalloc(e, &e->vprev, N * R_)) ||
        (st = dalloc(e, &e->gwin, 10 * N * R_)) || (st = dalloc(e, &e->act, 3 * N * R_)) ||
        (st = dalloc(e, &e->wind, 6 * N * R_)) || (st = dalloc(e, (void**)&e->ghead, N)) ||
        (st = dalloc(e, (void**)&e->glen, N)) || (st = dalloc(e, (void**)&e->wprof, N)) ||
        (st = dalloc(e, (void**)&e->key, 2 * N * 8)) || (st = dalloc(e, (void**)&e->slot, 2 * N * 4)) ||
        (st = dalloc(e, (void**)&e->tid, N)) || (st = dalloc(e, (void**)&e->epi, N * 4)) ||
        (st = dalloc(e, (void**)&e->tstep, N * 4)) || (st = dalloc(e, (void**)&e->fin, N)) ||
        (st = dalloc(e, (void**)&e->live[0], N * 4)) ||
        (st = dalloc(e, (void**)&e->live[1], N * 4)) || (st = dalloc(e, (void**)&e->live_cnt, 3 * 4)))
        return st;
    PD_HIP(hipMemset(e->gwin, 0, 10 * N * R_));
    PD_HIP(hipMemset(e->epi, 0xff, N * 4));   // first reset -> episode 0
    const unsigned long long stats0[kStats] = {0, 0, (unsigned long long)H.cd.entries, (unsigned long long)H.cl.entries};
    if ((st = dalloc(e, (void**)&e->pend.count, 8)) || (st = dalloc(e, (void**)&e->pend.keys, kPendingCap * 8)) ||
        (st = dalloc(e, (void**)&e->pend.pay, (size_t)kPendingCap * kPay * 8)) ||
        (st = upload(e, stats0, kStats, &e->pend.stats)) ||
        (st = dalloc(e, (void**)&e->pend.solve_ws, (size_t)kSolveSlots * kScratch * 8)) ||
        (st = dalloc(e, (void**)&e->pend.solve_lock, (size_t)kSolveSlots * 4)) ||
        (st = dalloc(e, (void**)&e->pend.ticket, 4)))
        return st;
    PD_HIP(hipMemset(e->pend.count, 0, 8));
    PD_HIP(hipMemset(e->pend.ticket, 0, 4));
    PD_HIP(hipMemset(e->pend.solve_lock, 0, (size_t)kSolveSlots * 4));
    // the policy rollouts' pinned live-count words and events, made here: a first pinned
    // allocation inside a timed rollout cost ~170 ms (the PSO driver's share handle)
    PD_HIP(hipHostMalloc((void**)&e->host_cnt, 2 * sizeof(uint32_t), hipHostMallocDefault));
    for (hipEvent_t& ev : e->cnt_ev) PD_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    StepArgs<R> a = make_args<R>(e);
    unsigned grid = (unsigned)((N + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_reset<R>, dim3(grid), dim3(kBlock), 0, 0, a, (const uint8_t*)nullptr);
    PD_HIP(hipGetLastError());
    PD_HIP(hipDeviceSynchronize());
    return PD_OK;
}

template <typename R, int PH, int RT, bool W> void launch_lpe(int lpe, const StepArgs<R>& a, hipStream_t s) {
    switch (lpe) {
        case 1: launch_step<R, PH, RT, W, 1>(a, s); break;
        case 2: launch_step<R, PH, RT, W, 2>(a, s); break;
        case 8: launch_step<R, PH, RT, W, 8>(a, s); break;
        case 16: launch_step<R, PH, RT, W, 16>(a, s); break;
        default: launch_step<R, PH, RT, W, 4>(a, s); break;
    }
}

template <typename R> void dispatch_step(const pd_env* e, const StepArgs<R>& a, hipStream_t s) {
    int ph = e->cfg.phase, l = e->lpe;
    bool pso = e->cfg.rtd == PD_RTD_PSO;   // RL and NONE share the RL instantiation (NONE zeroes the rtd)
    bool w = e->cfg.enable_wind != 0;
    if (e->cfg.integrator == PD_INTEG_RK4) {   // pure throttle, no wind (validated); LPE 2 or 16
        if (pso) { if (l <= 2) launch_step<R, 0, 1, false, 2, true>(a, s); else launch_step<R, 0, 1, false, 16, true>(a, s); }
        else { if (l <= 2) launch_step<R, 0, 0, false, 2, true>(a, s); else launch_step<R, 0, 0, false, 16, true>(a, s); }
        return;
    }
    if (ph == 0 && !pso) { if (w) launch_lpe<R, 0, 0, true>(l, a, s); else launch_lpe<R, 0, 0, false>(l, a, s); }
    else if (ph == 0) { if (w) launch_lpe<R, 0, 1, true>(l, a, s); else launch_lpe<R, 0, 1, false>(l, a, s); }
    else if (ph == 1 && pso) { if (w) launch_lpe<R, 1, 1, true>(l, a, s); else launch_lpe<R, 1, 1, false>(l, a, s); }
    else if (ph == 1) { if (w) launch_lpe<R, 1, 0, true>(l, a, s); else launch_lpe<R, 1, 0, false>(l, a, s); }
    else { if (w) launch_lpe<R, 2, 0, true>(l, a, s); else launch_lpe<R, 2, 0, false>(l, a, s); }
}

// Policy rollouts run at 2 lanes per env whatever the handle's step LPE: the per-lane actor and
// the LPE 2 table path (Taylor lines, cell pieces) fit 256 VGPRs without scratch.
// pd_tuning.policy_lanes 4/8 (the c4 lanes-per-env sweep) runs the LPE 4/8 instantiations, whose
// tables take the split payload sums.
template <typename R, int PH, bool W> void launch_policy(int lpe, const StepArgs<R>& a, int64_t n_launch, hipStream_t s) {
    switch (lpe) {
        case 4: launch_policy_lpe<R, PH, W, 4>(a, n_launch, s); break;
        case 8: launch_policy_lpe<R, PH, W, 8>(a, n_launch, s); break;
        default: launch_policy_lpe<R, PH, W, 2>(a, n_launch, s); break;
    }
}

// the handle's (landing-burn phase, wind) instantiation of the policy rollout kernels
template <typename R> void dispatch_policy(const pd_env* e, const StepArgs<R>& a, int64_t n_launch, hipStream_t s) {
    const int l = e->tune.policy_lanes;
    const bool w = e->cfg.enable_wind != 0;
    if (e->cfg.phase == PD_PHASE_PURE_THROTTLE) { if (w) launch_policy<R, 0, true>(l, a, n_launch, s); else launch_policy<R, 0, false>(l, a, n_launch, s); }
    else { if (w) launch_policy<R, 1, true>(l, a, n_launch, s); else launch_policy<R, 1, false>(l, a, n_launch, s); }
}

// and of the SAC rollout kernels
template <typename R> void dispatch_sac_roll(const pd_env* e, const StepArgs<R>& a, hipStream_t s) {
    const bool w = e->cfg.enable_wind != 0;
    if (e->cfg.phase == PD_PHASE_PURE_THROTTLE) { if (w) launch_sac_roll<R, 0, true>(a, s); else launch_sac_roll<R, 0, false>(a, s); }
    else { if (w) launch_sac_roll<R, 1, true>(a, s); else launch_sac_roll<R, 1, false>(a, s); }
}

// and of the SAC collection kernels
template <typename R> void dispatch_sac_collect(const pd_env* e, const StepArgs<R>& a, hipStream_t s) {
    const bool w = e->cfg.enable_wind != 0;
    if (e->cfg.phase == PD_PHASE_PURE_THROTTLE) { if (w) launch_sac_collect<R, 0, true>(a, s); else launch_sac_collect<R, 0, false>(a, s); }
    else { if (w) launch_sac_collect<R, 1, true>(a, s); else launch_sac_collect<R, 1, false>(a, s); }
}

template <typename R> void launch_insert(pd_env* e, hipStream_t s) {
    hipLaunchKernelGGL(k_insert<R>, dim3(1), dim3(64), 0, s, e->pend, e->keys_cd, (R*)e->pay_cd, e->logcap_cd,
                       e->keys_cl, (R*)e->pay_cl, e->logcap_cl);
}

// pd_step_sac's inputs and float32 outputs (see include/pdenv.h)
struct SacIO {
    const float *mean, *log_std, *eps;
    float lo, hi, max_action;
    float *action, *slab, *obs32;
    uint32_t head_stride;
    // pd_step_sac_ring
    int draw = 0;
    float* eps_out = nullptr;
    int64_t ring_cap = 0;
    long long* ring_state = nullptr;
    float* prio = nullptr;
    const float* max_prio = nullptr;
    // pd_step_sac_fused: the actor in the kernel prologue (mlp.H = 0: off)
    SacMlp mlp{};
    float* heads_out = nullptr;
};

// a step launch's outputs (device memory; null: not written)
struct StepOut {
    void *obs = nullptr, *reward = nullptr;
    uint8_t *done = nullptr, *trunc = nullptr;
    int8_t* tid = nullptr;
    void* info = nullptr;
    uint64_t info_mask = (1ull << PD_N_INFO) - 1ull;
    void* reward_sum = nullptr;
};

template <typename R>
pd_status step_impl(pd_env* e, const void* actions, const StepOut& o, hipStream_t s, int n_fused = 1,
                    const double* noise = nullptr, const SacIO* sac = nullptr) {
    // every caller's launch needs its inputs: actions (plain steps), the heads or the actor (SAC);
    // the public entry points check them too, this keeps an internal caller from launching a
    // kernel that would read through a null pointer
    if (!sac && !actions) return fail(PD_ERR_INVALID, "step launch without actions");
    if (sac && sac->mlp.H == 0 && !sac->mean) return fail(PD_ERR_INVALID, "SAC step launch without heads or actor");
    if (sac && sac->mlp.H != 0 && (!sac->mlp.obs || !sac->mlp.wm || !sac->mlp.ws))
        return fail(PD_ERR_INVALID, "SAC step launch with an incomplete actor");
    if (sac && (e->cfg.rtd == PD_RTD_PSO || e->cfg.integrator != PD_INTEG_REFERENCE ||
                (e->cfg.phase != PD_PHASE_PURE_THROTTLE && e->cfg.phase != PD_PHASE_LANDING_BURN)))
        return fail(PD_ERR_UNSUPPORTED, "SAC step launch on a handle without a SAC kernel");
    StepArgs<R> a = make_args<R>(e);
    a.actions = actions; a.obs = (R*)o.obs; a.reward = (R*)o.reward; a.done = o.done; a.trunc = o.trunc; a.trunc_id = o.tid;
    a.noise = noise; a.info = (R*)o.info; a.reward_sum = (R*)o.reward_sum;
    a.info_mask = o.info_mask; a.info_nsel = __builtin_popcountll(o.info_mask);
    a.n_fused = n_fused;
    if (sac) {
        a.sac_mean = sac->mean; a.sac_logstd = sac->log_std; a.sac_eps = sac->eps;
        a.sac_lo = sac->lo; a.sac_hi = sac->hi; a.sac_max = sac->max_action;
        a.sac_act = sac->action; a.slab = sac->slab; a.obs32 = sac->obs32;
        a.sac_hs = sac->head_stride;
        a.sac_draw = sac->draw; a.sac_eps_out = sac->eps_out;
        a.ring_cap = sac->ring_cap; a.ring_state = sac->ring_state; a.prio = sac->prio; a.max_prio = sac->max_prio;
        a.sac_mlp = sac->mlp; a.sac_heads_out = sac->heads_out;
    }
    dispatch_step<R>(e, a, s);
    PD_HIP(hipGetLastError());
    return PD_OK;
}

// the SAC entry points' launch: one step, every output in io
pd_status sac_step(pd_env* e, const SacIO& io, void* stream) {
    return with_real(e, [&](auto r) { return step_impl<decltype(r)>(e, nullptr, StepOut{}, (hipStream_t)stream, 1, nullptr, &io); });
}

// pd_rollout_sac: whole episodes driven by the actor inside the step loop (k_step<..., SAC, ROLL>),
// a chain of launches of at most pd_tuning.step_fuse steps -- each launch's last workgroup
// inserts the neighbourhoods it solved, as in pd_step_n -- with no host synchronisation: a later
// launch reads the b.fin flags, and a workgroup with no live env only falls through to the ticket
template <typename R>
pd_status rollout_sac_impl(pd_env* e, const SacIO& io, int reset_first, int32_t max_steps, void* ret, int32_t* steps,
                           uint8_t* done, int8_t* tid, float* actions_out, void* rewards_out, hipStream_t s) {
    const size_t N = (size_t)e->cfg.n_envs;
    if (!ret) {
        if (!e->roll_ret) {
            PD_HIP(hipMalloc(&e->roll_ret, N * 8));
            e->allocs.push_back(e->roll_ret);
        }
        ret = e->roll_ret;
    }
    if (reset_first) {   // pd_reset of every env (clears b.fin)
        hipLaunchKernelGGL(k_reset<R>, dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, make_args<R>(e),
                           (const uint8_t*)nullptr);
        PD_HIP(hipGetLastError());
    } else {
        PD_HIP(hipMemsetAsync(e->fin, 0, N, s));
    }
    PD_HIP(hipMemsetAsync(ret, 0, N * sizeof(R), s));
    if (steps) PD_HIP(hipMemsetAsync(steps, 0, N * 4, s));
    if (done) PD_HIP(hipMemsetAsync(done, 0, N, s));
    // (an env that takes no step keeps the trunc_id its last step left)
    if (tid) PD_HIP(hipMemcpyAsync(tid, e->tid, N, hipMemcpyDeviceToDevice, s));
    const int K = e->tune.step_fuse;
    for (int32_t t = 0; t < max_steps; t += K) {
        StepArgs<R> a = make_args<R>(e);
        a.n_fused = max_steps - t < K ? max_steps - t : K;
        a.sac_lo = io.lo; a.sac_hi = io.hi; a.sac_max = io.max_action;
        a.sac_hs = io.head_stride; a.sac_draw = io.draw; a.sac_mlp = io.mlp;
        a.roll_t0 = t;
        a.roll_ret = (R*)ret; a.roll_steps = steps; a.roll_done = done; a.roll_tid = tid;
        a.roll_act = actions_out; a.roll_rew = (R*)rewards_out;
        dispatch_sac_roll<R>(e, a, s);
        PD_HIP(hipGetLastError());
    }
    // (b.fin means "frozen until reset" to the policy rollouts: left clear for whatever follows)
    PD_HIP(hipMemsetAsync(e->fin, 0, N, s));
    return PD_OK;
}

// pd_collect_sac: n_steps collection steps (k_step<..., SAC, kRollCollect>) as a chain of launches
// of at most pd_tuning.step_fuse steps, with no host synchronisation and no allocation.  Each
// launch's per-step outputs (and, slab mode, its rows) start at the steps already taken; in ring
// mode every launch reads the ring's position from ring_state and its last workgroup advances it
template <typename R>
pd_status collect_sac_impl(pd_env* e, const SacIO& io, int32_t n_steps, void* reward, uint8_t* done, uint8_t* trunc,
                           int8_t* tid, hipStream_t s) {
    const size_t N = (size_t)e->cfg.n_envs, A = (size_t)e->act_dim;
    const size_t W = 2 * (size_t)e->obs_dim + A + 2;
    const int K = e->tune.step_fuse;
    for (int32_t t = 0; t < n_steps; t += K) {
        StepArgs<R> a = make_args<R>(e);
        a.n_fused = n_steps - t < K ? n_steps - t : K;
        a.sac_lo = io.lo; a.sac_hi = io.hi; a.sac_max = io.max_action;
        a.sac_hs = io.head_stride; a.sac_draw = io.draw; a.sac_mlp = io.mlp;
        a.sac_eps_out = io.eps_out ? io.eps_out + (size_t)t * N * A : nullptr;
        a.slab = io.ring_state ? io.slab : io.slab + (size_t)t * N * W;
        a.obs32 = io.obs32;
        a.ring_cap = io.ring_cap; a.ring_state = io.ring_state; a.prio = io.prio; a.max_prio = io.max_prio;
        a.reward = reward ? (R*)reward + (size_t)t * N : nullptr;
        a.done = done ? done + (size_t)t * N : nullptr;
        a.trunc = trunc ? trunc + (size_t)t * N : nullptr;
        a.trunc_id = tid ? tid + (size_t)t * N : nullptr;
        dispatch_sac_collect<R>(e, a, s);
        PD_HIP(hipGetLastError());
    }
    return PD_OK;
}

// policy rollouts: the caller's parameter-major weights [P][N] in chunks of four parameters,
// [ceil(P / 4)][N][4] (zeros past P), the layout actor_forward reads with one 16-byte load per
// chunk (pd_step_impl.h)
__global__ __launch_bounds__(kBlock) void k_wchunk(const float* __restrict__ w, float4* __restrict__ out, int P,
                                                   int64_t N) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t C = (P + 3) / 4;
    if (t >= C * N) return;
    const int c = (int)(t / N);
    const int64_t i = t - (int64_t)c * N;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = 4 * c + k < P ? w[(int64_t)(4 * c + k) * N + i] : 0.f;
    out[t] = make_float4(v[0], v[1], v[2], v[3]);
}

// policy rollouts' prologue in one launch: k_reset of every env, its fitness zeroed, every env
// live in index order (the list, count 0 = n and the other two counts zero; refill: the three
// counts zero, the refill launch's hand-out counter among them) -- the four launches a rollout
// used to start with
template <typename R>
__global__ __launch_bounds__(kBlock) void k_policy_init(StepArgs<R> a, R* __restrict__ fitness, int32_t* list,
                                                        uint32_t* cnt, int refill) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < 3) cnt[i] = (i == 0 && !refill) ? (uint32_t)a.n : 0u;
    if (i >= a.n) return;
    list[i] = (int32_t)i;
    fitness[i] = R(0);
    DP<R>& P = *params<R>(a.P);
    const uint32_t ui = (uint32_t)i;
    EnvRegs<R> e;
    reset_values<R>(P, a, a.env_offset + (uint64_t)i, ev(a.b.epi, ui) + 1u,
                    (const double*)(uint64_t)&P.logtab.invc[0], (const double*)(uint64_t)&P.logtab.logc[0], e);
    store_env<R>(a, P, ui, e, true);
}

// policy rollouts' epilogue in one launch: k_insert (thread 0 of block 0) and the episode lengths
// copied to the caller's steps (the tstep words), which used a copy of its own
template <typename R>
__global__ __launch_bounds__(kBlock) void k_policy_finish(Pending pend, unsigned long long* keys_cd, R* pay_cd,
                                                          int lc_cd, unsigned long long* keys_cl, R* pay_cl, int lc_cl,
                                                          const uint32_t* __restrict__ tstep, int32_t* __restrict__ steps,
                                                          int64_t n) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
        insert_pending<R>(pend.count, pend.keys, pend.pay, pend.stats, keys_cd, pay_cd, lc_cd, keys_cl, pay_cl, lc_cl);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (steps && i < n) steps[i] = (int32_t)tstep[i];
}

template <typename R> void launch_policy_finish(pd_env* e, int32_t* steps, hipStream_t s) {
    const int64_t N = e->cfg.n_envs;
    hipLaunchKernelGGL(k_policy_finish<R>, dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, e->pend,
                       e->keys_cd, (R*)e->pay_cd, e->logcap_cd, e->keys_cl, (R*)e->pay_cl, e->logcap_cl,
                       (const uint32_t*)e->tstep, steps, N);
}

template <typename R>
pd_status rollout_policy_impl(pd_env* e, const float* w, int32_t max_steps, void* fitness, int32_t* steps,
                              int32_t check_every, hipStream_t s, bool chunked = false) {
    const int64_t N = e->cfg.n_envs;
    unsigned grid = (unsigned)((N + kBlock - 1) / kBlock);
    // the weights in the chunked layout of the step kernel's actor (one pass over them: 2 x 1.5 KB
    // per particle, against the 1.5 KB per policy step the rollout reads), unless the caller's
    // are chunked already (pd_rollout_policy_chunked: pd_pso_step_chunked writes that layout)
    const int P = e->cfg.phase == PD_PHASE_PURE_THROTTLE ? PD_ACTOR_PARAMS_PURE_THROTTLE : PD_ACTOR_PARAMS_LANDING_BURN;
    if (!chunked) {
        if (!e->pol_w4) {
            PD_HIP(hipMalloc((void**)&e->pol_w4, (size_t)PD_ACTOR_PARAMS_LANDING_BURN * (size_t)N * sizeof(float)));
            e->allocs.push_back(e->pol_w4);
        }
        const int64_t tot = (int64_t)((P + 3) / 4) * N;
        hipLaunchKernelGGL(k_wchunk, dim3((unsigned)((tot + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, w,
                           (float4*)e->pol_w4, P, N);
    }
    StepArgs<R> a = make_args<R>(e);
    a.policy_w = chunked ? w : e->pol_w4; a.reward_sum = (R*)fitness; a.auto_reset = 0;
    const bool wind = e->cfg.enable_wind != 0;
    // launch t steps live[t & 1][0, live_cnt[t % 3]) and appends the survivors to the other list;
    // the grid covers the live count last read back (a workgroup past the device count leaves
    // at once), so the launches shrink with the swarm's live envs.  Checks are one interval
    // behind: at a check the count is copied to pinned memory under an event, and the host
    // waits for the PREVIOUS check's event, with check_every launches still queued behind it
    // (no bubble); at most 2 * check_every nearly empty launches run after the last episode.
    if (check_every > 0 && !e->host_cnt) return fail(PD_ERR_HIP, "policy rollout: no pinned live-count words");
    // The list pays off once the grid no longer fits the chip in one round (a launch then costs
    // the rounds its waves need); below that the launch time is one wave's, and reading the
    // state and actor weights through the list (gathers) only costs.  pd_tuning.policy_list forces.
    int dev_cus = 256;
    (void)hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, e->device);
    const int plpe = e->tune.policy_lanes;
    // refill: one launch of the chip's resident env slots (two waves per SIMD) steps the whole
    // swarm, the lanes of an ended episode taking the next particle -- the grid's lanes stay busy
    // until the swarm's last particles, where a launch per live-list check leaves most of a
    // workgroup's lanes idle behind its longest episode
    const int64_t cap = (int64_t)dev_cus * 512 / plpe;
    // (auto: a wave's slots are handed particles once three quarters of them wait -- 24 of the 32
    // at two lanes per env: c4 at 262 144 particles 4.71 ms a rollout, against 12.4 / 8.6 / 6.5 /
    // 5.5 / 5.0 / 5.0 ms at batches of 1 / 4 / 8 / 12 / 16 / 32 and 5.94 ms without refill)
    const int kRefillBatch = 48 / plpe;
    // (windless handles only: the windy policy kernels compile no refill, see pd_step_impl.h)
    // (and a swarm of at least one wave's slots: the slots are whole waves, none past the swarm).
    // Auto: every windless swarm -- beyond the resident slots for the refills, and within them for
    // the one launch without live-count reads (c4 at 32 768 particles: 1.452 ms a generation
    // against 1.476 with the per-check launches, profiles/r05_c4_refill.jsonl)
    // (auto refill yields to an explicit request for the per-check launches: policy_list >= 0 or
    // policy_list_at > 0 with policy_refill -1; check_every and the list apply to those only)
    const bool refill_on = e->tune.policy_refill > 0 ||
                           (e->tune.policy_refill < 0 && e->tune.policy_list < 0 && !(e->tune.policy_list_at > 0.0));
    const bool refill = !wind && N >= 64 / plpe && refill_on;
    // every env reset, fitness zeroed, the live list and counts initialised: one launch
    hipLaunchKernelGGL(k_policy_init<R>, dim3(grid), dim3(kBlock), 0, s, make_args<R>(e), (R*)fitness, e->live[0],
                       e->live_cnt, refill ? 1 : 0);
    if (refill) {
        // slots: whole waves (epw envs each), at most the swarm; wave w owns particles
        // [w Q, (w + 1) Q) -- its first epw are its slots' first episodes -- and takes them
        // without atomics; the rest, from waves x Q on, is the shared pool (batched hand-outs).
        // Q: policy_refill_own percent of the swarm over the waves, whole waves' worth of envs
        // (default 100: c4 at 262 144 particles, 128 per wave, no pool -- 3.97 ms a rollout against
        // 4.22 / 4.18 / 4.54 / 4.75 ms with 90 / 75 / 50 / 0 % own, the rest from the pool in
        // batches of 24: the pool's batching idles more lanes than the waves' uneven work does)
        const int64_t epw = 64 / plpe;
        int64_t slots = std::min<int64_t>(N, e->tune.policy_slots > 0 ? e->tune.policy_slots : cap);
        slots = std::max<int64_t>(epw, slots / epw * epw);   // (<= N: N >= epw)
        const int64_t waves = slots / epw;
        const int own = e->tune.policy_refill_own >= 0 ? e->tune.policy_refill_own : 100;
        int64_t q = (int64_t)((double)N * own / 100.0 / (double)waves) / epw * epw;
        q = std::max<int64_t>(epw, std::min<int64_t>(q, N / waves / epw * epw));   // (waves q <= N: N >= slots)
        a.use_list = 0; a.policy_wc = nullptr;
        a.refill = e->tune.policy_refill > 0 ? e->tune.policy_refill : kRefillBatch;
        a.refill_next = e->live_cnt; a.refill_max = max_steps;
        a.refill_slots = (int)slots; a.refill_q = (int)q; a.refill_base = (int)(waves * q);
        a.list_in = e->live[0]; a.list_out = e->live[1];
        a.cnt_in = e->live_cnt + 1; a.cnt_out = e->live_cnt + 1; a.cnt_zero = e->live_cnt + 2;
        // (a bound every wave reaches: a wave runs at most its own q particles and the pool's,
        // one of its slots live at every step until they are all handed out, each episode at most
        // max_steps steps; the waves leave when their lanes have none left)
        const int64_t bound = (int64_t)max_steps * (q + (N - waves * q) + 1);
        a.n_fused = (int)std::min<int64_t>(bound, INT32_MAX);
        dispatch_policy<R>(e, a, slots, s);
        PD_HIP(hipGetLastError());
        launch_policy_finish<R>(e, steps, s);
        PD_HIP(hipGetLastError());
        return PD_OK;
    }
    a.use_list = e->tune.policy_list >= 0 ? e->tune.policy_list : (N * plpe > (int64_t)dev_cus * 512);
    // every launch appends its survivors to the next list, so the rollout can switch to the list
    // at any launch: once the live count read back falls to policy_list_at x N (default off), the
    // waves of the later launches hold live envs only
    const double compact_at = e->tune.policy_list_at;
    // the list launches' parameter copy (policy_wc, chunked as pol_w4): made at the first rollout
    if (!e->pol_wc) {
        PD_HIP(hipMalloc((void**)&e->pol_wc, (size_t)PD_ACTOR_PARAMS_LANDING_BURN * (size_t)N * sizeof(float)));
        e->allocs.push_back(e->pol_wc);
    }
    a.policy_wc = e->pol_wc;
    int64_t n_launch = N;
    int checks = 0;
    // F policy steps per launch (an episode that ends inside a launch is stored at its last step
    // and its lanes freeze); the live list is compacted once per launch
    const int F = e->tune.policy_fuse;
    const int check_launches = check_every > 0 ? std::max(1, check_every / F) : 0;
    int32_t t = 0;
    for (int l = 0; t < max_steps; ++l) {
        a.n_fused = std::min<int32_t>(F, max_steps - t);
        t += a.n_fused;
        a.list_in = e->live[l & 1]; a.list_out = e->live[(l + 1) & 1];
        a.cnt_in = e->live_cnt + l % 3; a.cnt_out = e->live_cnt + (l + 1) % 3; a.cnt_zero = e->live_cnt + (l + 2) % 3;
        dispatch_policy<R>(e, a, n_launch, s);
        PD_HIP(hipGetLastError());
        if (F >= 16 || (l & (16 / F - 1)) == 16 / F - 1) launch_insert<R>(e, s);
        if (check_launches > 0 && (l + 1) % check_launches == 0 && t < max_steps) {
            const int k = checks & 1;
            PD_HIP(hipMemcpyAsync(e->host_cnt + k, e->live_cnt + (l + 1) % 3, 4, hipMemcpyDeviceToHost, s));
            PD_HIP(hipEventRecord(e->cnt_ev[k], s));
            if (checks > 0) {
                PD_HIP(hipEventSynchronize(e->cnt_ev[k ^ 1]));
                const uint32_t live = ((volatile uint32_t*)e->host_cnt)[k ^ 1];
                if (live == 0) break;
                if (!a.use_list && compact_at > 0.0 && (double)live <= compact_at * (double)N) a.use_list = 1;
                if (a.use_list) n_launch = live;
            }
            ++checks;
        }
    }
    launch_policy_finish<R>(e, steps, s);
    PD_HIP(hipGetLastError());
    return PD_OK;
}

// Launch tuning defaults (pd_tuning).  policy_fuse 64: a wave whose episodes have all ended leaves
// its launch, so a longer launch costs no frozen steps at the swarm's tail; it saves launches,
// their table staging and the count checks between them (c4: 8 -> 1.66, 16 -> 1.57, 32 ->
// 1.53-1.57, 64 -> 1.49-1.50 ms per generation, profiles/r04_exp_s16_pol_exit.jsonl,
// r04_exp_s17_pfuse.jsonl).  step_fuse 128: the miss flush runs between launches, so a
// neighbourhood solved on device is re-solved at most this many steps before it is in the tables
// (c3 ms per env-step, payload sums: 16 -> 0.0450, 32 -> 0.0442, 64 -> 0.0421; cell pieces: 64 ->
// 0.0341, 128 -> 0.0335, 256 -> 0.0337).

// n_steps env-steps in launches of pd_tuning.step_fuse fused steps (each inserts its own misses).
// Row t of every [n_steps][N...] array belongs to step t; NULL outputs are not written.
pd_status step_n_impl(pd_env* e, const void* actions, int32_t n_steps, void* obs, void* reward, uint8_t* done,
                      uint8_t* trunc, int8_t* tid, void* reward_sum, hipStream_t s, void* info = nullptr,
                      uint64_t info_mask = 0) {
    const size_t N = (size_t)e->cfg.n_envs;
    const size_t sa = N * e->act_dim * (e->cfg.action_f64 ? 8 : 4), so = N * e->obs_dim * e->rsize;
    const size_t sr = N * e->rsize;
    const size_t si = N * e->rsize * (size_t)__builtin_popcountll(info_mask);   // one step's info rows
    const int K = e->tune.step_fuse;
    for (int32_t t = 0; t < n_steps; t += K) {
        const int k = n_steps - t < K ? n_steps - t : K;
        auto at = [&](void* p, size_t stride) { return p ? (void*)((char*)p + stride * t) : nullptr; };
        const void* act = (const char*)actions + sa * t;
        const StepOut o{at(obs, so), at(reward, sr), (uint8_t*)at(done, N), (uint8_t*)at(trunc, N), (int8_t*)at(tid, N),
                        at(info, si), info_mask, reward_sum};
        pd_status st = with_real(e, [&](auto r) { return step_impl<decltype(r)>(e, act, o, s, k); });
        if (st != PD_OK) return st;
        // (no miss flush between the launches: each step launch's last workgroup inserts the
        // neighbourhoods its launch solved, k_step's tail)
    }
    return PD_OK;
}

}  // namespace

// ================================================================ C ABI
extern "C" {

int pd_abi_version(void) { return PD_ABI_VERSION; }

extern "C++" {
namespace {
// the device's table evaluation (atmosphere<R, true>, pd_physics.h) on the host, in R
template <typename R>
void eval_atm_table(const pd_params* p, const double* alt, int64_t n_alt, double* atm_out, double* max_rel) {
    std::vector<R> atm;
    int n_atm = 0;
    build_atm_table<R>(p, atm, n_atm, *max_rel);
    for (int64_t i = 0; i < n_alt; ++i) {
        R y = (R)alt[i], al = y < R(0) ? R(0) : y, out[3] = {R(0), R(0), R(0)};
        if (al < (R)p->isa_alt_max) {
            int k = (int)(al * (R)(1.0 / kAtmW));
            k = k > n_atm - 1 ? n_atm - 1 : k;
            const R* rec = atm.data() + (size_t)k * kAtmStride;
            if (rec[1] < R(1e29) && (R)p->isa_r * al / ((R)p->isa_r + al) >= rec[1]) rec += kAtmRec;
            const R t = al - rec[0];
            for (int fn = 0; fn < 3; ++fn) out[fn] = horner_host<R>(rec + 2 + fn * (kAtmDeg + 1), kAtmDeg, t);
        }
        atm_out[3 * i] = (double)out[1]; atm_out[3 * i + 1] = (double)out[0]; atm_out[3 * i + 2] = (double)out[2];
    }
}
}  // namespace
}  // extern "C++"

pd_status pd_atm_table(const pd_params* p, int32_t precision, const double* alt, int64_t n_alt, double* atm_out,
                       double* max_rel) {
    if (!p || !max_rel || n_alt < 0 || (n_alt && (!alt || !atm_out))) return fail(PD_ERR_INVALID, "pd_atm_table: bad arguments");
    with_real(precision != PD_F32, [&](auto r) { eval_atm_table<decltype(r)>(p, alt, n_alt, atm_out, max_rel); });
    return PD_OK;
}
// the coarse LDS table (atmosphere_lds, pd_physics.h) on the host, in binary64, in the device's order
pd_status pd_atm_table_lds(const pd_params* p, const double* alt, int64_t n_alt, double* atm_out, double* max_rel,
                           int32_t* n_cells_out) {
    if (!p || !max_rel || n_alt < 0 || (n_alt && (!alt || !atm_out))) return fail(PD_ERR_INVALID, "pd_atm_table_lds: bad arguments");
    std::vector<double> atl;
    int n_cells = 0, n_rec = 0;
    build_atm_lds_table<double>(p, atl, n_cells, n_rec, *max_rel);
    if (n_cells_out) *n_cells_out = n_cells;
    if (!(*max_rel <= 1e-14)) return fail(PD_ERR_UNSUPPORTED, "pd_atm_table_lds: the table is past 1e-14 (handles take the exact formulas)");
    const double inv_w = 1.0 / kAtlW;
    for (int64_t i = 0; i < n_alt; ++i) {
        const double y = alt[i], al = y < 0.0 ? 0.0 : y;
        double out[3] = {0.0, 0.0, 0.0};
        if (al < p->isa_alt_max) {
            int k = (int)(al * inv_w);
            k = k > n_cells - 1 ? n_cells - 1 : k;
            const double* rec = atl.data() + (size_t)k * kAtlStride;
            if (rec[1] < 1e29 && p->isa_r * al / (p->isa_r + al) >= rec[1]) rec = atl.data() + (size_t)(int)rec[kAtlRec - 1] * kAtlStride;
            const double t = al - rec[0];
            for (int fn = 0; fn < 3; ++fn) out[fn] = horner_host<double>(rec + 2 + fn * (kAtlDeg + 1), kAtlDeg, t);
        }
        atm_out[3 * i] = out[1]; atm_out[3 * i + 1] = out[0]; atm_out[3 * i + 2] = out[2];
    }
    return PD_OK;
}
// the wind profiles' interval slopes as the 512-thread kernels' LDS image tabulates them
// (pd_step.h wind_slope), binary64: out [PD_N_WIND_PROFILES][PD_MAX_WIND]
pd_status pd_wind_slopes(const pd_params* p, double* out) {
    if (!p || !out) return fail(PD_ERR_INVALID, "pd_wind_slopes: bad arguments");
    static_assert(PD_N_WIND_PROFILES * PD_MAX_WIND == 800, "wind profile tables");
    auto D = std::make_unique<DevParams<double>>();
    for (int w = 0; w < PD_N_WIND_PROFILES; ++w) {
        D->wind_n[w] = p->wind_n[w];
        for (int j = 0; j < PD_MAX_WIND; ++j) { D->wind_alt_km[w][j] = p->wind_alt_km[w][j]; D->wind_speed[w][j] = p->wind_speed[w][j]; }
    }
    for (int t = 0; t < 800; ++t) out[t] = wind_slope<double>(*D, t / PD_MAX_WIND, t % PD_MAX_WIND);
    return PD_OK;
}
pd_status pd_cell_piece_info(const pd_params* p, int32_t table, int64_t piece, double* out, int32_t n_out) {
    if (!p || !out || n_out < 16 || (table != 0 && table != 1)) return fail(PD_ERR_INVALID, "pd_cell_piece_info: bad arguments");
    const pd_aero_table& t = table ? p->cl : p->cd;
    if (t.n_pts < kNbr || t.n_pts > PD_MAX_PTS || t.n_cols != kCols) return fail(PD_ERR_INVALID, "pd_cell_piece_info: bad table");
    int nm, na;
    double a0, a1;
    grid_geometry(table, nm, na, a0, a1);
    CellPieces& cp = const_cast<CellPieces&>(cell_pieces(t, a0, a1, nm, na));
    ensure_f32(cp);
    int64_t ok32 = 0;
    for (uint8_t c : cp.cell_ok32) ok32 += c;
    int64_t ok64 = 0;
    for (uint8_t c : cp.cell_ok) ok64 += c;
    const double v[16] = {(double)cp.pieces, (double)cp.rejected, cp.max_rel, cp.build_s, (double)(cp.rec.size() / kCellStride),
                          (double)nm, (double)na, a0, a1, (double)kCellDeg, (double)kCellExact, (double)kCellStride,
                          (double)cp.rejected32, cp.max_rel32, (double)ok64, (double)ok32};
    for (int k = 0; k < 16; ++k) out[k] = v[k];
    if (piece >= 0) {
        if ((size_t)(piece + 1) * kCellStride > cp.rec.size() || n_out < 16 + kCellStride)
            return fail(PD_ERR_INVALID, "pd_cell_piece_info: piece out of range or out too short");
        std::memcpy(out + 16, cp.rec.data() + (size_t)piece * kCellStride, kCellStride * sizeof(double));
    }
    return PD_OK;
}

size_t pd_sizeof_params(void) { return sizeof(pd_params); }
size_t pd_sizeof_config(void) { return sizeof(pd_config); }
const char* pd_last_error(void) { return g_err.c_str(); }

int pd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

pd_status pd_create(const pd_params* params, const pd_config* cfg, pd_env** out) {
    if (!out) return fail(PD_ERR_INVALID, "out is null");
    *out = nullptr;
    pd_status st = validate(params, cfg);
    if (st != PD_OK) return st;
    int ndev = pd_device_count();
    if (ndev <= 0) return fail(PD_ERR_HIP, "no HIP device visible");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(PD_ERR_INVALID, "device ordinal out of range");
    PD_HIP(hipSetDevice(cfg->device));
    pd_env* e = new pd_env();
    e->cfg = *cfg;
    e->device = cfg->device;
    e->act_dim = act_dim_of(cfg->phase);
    e->obs_kind = obs_kind_of(cfg->phase, cfg->rtd);
    e->obs_dim = obs_dim(e->obs_kind);
    e->rsize = cfg->precision == PD_F64 ? 8 : 4;
    // default lanes per env.  Below ~64k envs the step is bound by one wave's latency: splitting
    // each table's sum over LPE / 2 lanes shortens it, while LPE 2 alone has the Taylor lines,
    // cell pieces and fine index.  Measured on the round-3 kernels (f64 ms per
    // env-step, 128 steps per launch, wind / no wind; profiles/r03_exp_lpe_sweep.jsonl):
    //   4 096: LPE 16 0.0221 / 0.0186, 8 0.0242, 2 0.0261 / 0.0237
    //   8 192: LPE 8 0.0249 / 0.0210, 2 0.0260 / 0.0235, 4 0.0277 / 0.0241, 16 0.0274 / 0.0235
    //  16 384: LPE 2 0.0261 / 0.0234, 4 0.0277 / 0.0240, 8 0.0306
    //  32 768: LPE 2 0.0263, 4 0.0352; 65 536: LPE 2
    e->lpe = cfg->lanes_per_env != 0 ? cfg->lanes_per_env
                                     : (cfg->n_envs <= 4096 ? 16 : (cfg->n_envs <= 8192 ? 8 : 2));
    if (e->lpe != 1 && e->lpe != 2 && e->lpe != 4 && e->lpe != 8 && e->lpe != 16) { delete e; return fail(PD_ERR_INVALID, "lanes_per_env must be 0, 1, 2, 4, 8 or 16"); }
    if (cfg->integrator == PD_INTEG_RK4) e->lpe = e->lpe <= 2 ? 2 : 16;   // the RK4 instantiations
    st = with_real(e, [&](auto r) { return create_impl<decltype(r)>(params, cfg, e); });
    if (st != PD_OK) { pd_destroy(e); return st; }
    *out = e;
    return PD_OK;
}

pd_status pd_destroy(pd_env* e) {
    if (!e) return PD_OK;
    (void)hipSetDevice(e->device);
    for (void* p : e->allocs) (void)hipFree(p);
    if (e->host_cnt) (void)hipHostFree(e->host_cnt);
    for (hipEvent_t ev : e->cnt_ev) if (ev) (void)hipEventDestroy(ev);
    delete e;
    return PD_OK;
}

pd_status pd_set_tuning(pd_env* e, const pd_tuning* t) {
    if (!e || !t) return fail(PD_ERR_INVALID, "pd_set_tuning: null env/tuning");
    const int pf = t->policy_fuse;
    if (t->step_fuse < 1 || t->step_fuse > 256) return fail(PD_ERR_INVALID, "pd_set_tuning: step_fuse must be 1..256");
    if (pf < 1 || pf > 64 || (pf & (pf - 1))) return fail(PD_ERR_INVALID, "pd_set_tuning: policy_fuse must be a power of two 1..64");
    if (t->policy_lanes != 2 && t->policy_lanes != 4 && t->policy_lanes != 8)
        return fail(PD_ERR_INVALID, "pd_set_tuning: policy_lanes must be 2, 4 or 8");
    if (t->policy_list < -1 || t->policy_list > 1) return fail(PD_ERR_INVALID, "pd_set_tuning: policy_list must be -1, 0 or 1");
    if (!(t->policy_list_at >= 0.0 && t->policy_list_at <= 1.0))
        return fail(PD_ERR_INVALID, "pd_set_tuning: policy_list_at must be in [0, 1]");
    if (t->policy_refill < -1 || t->policy_refill > 64)
        return fail(PD_ERR_INVALID, "pd_set_tuning: policy_refill must be -1 (auto), 0 (off) or a batch of 1..64 slots");
    if (t->policy_slots < 0) return fail(PD_ERR_INVALID, "pd_set_tuning: policy_slots must be >= 0");
    if (t->policy_refill_own < -1 || t->policy_refill_own > 100)
        return fail(PD_ERR_INVALID, "pd_set_tuning: policy_refill_own must be -1 (auto) or a percentage 0..100");
    e->tune = *t;
    return PD_OK;
}

pd_status pd_get_tuning(const pd_env* e, pd_tuning* t) {
    if (!e || !t) return fail(PD_ERR_INVALID, "pd_get_tuning: null env/tuning");
    *t = e->tune;
    return PD_OK;
}

pd_status pd_reset(pd_env* e, const uint8_t* mask, void* obs, void* stream) {
    if (!e) return fail(PD_ERR_INVALID, "null env");
    PD_HIP(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    unsigned grid = (unsigned)((e->cfg.n_envs + kBlock - 1) / kBlock);
    with_real(e, [&](auto r) { using R = decltype(r); hipLaunchKernelGGL(k_reset<R>, dim3(grid), dim3(kBlock), 0, s, make_args<R>(e), mask); });
    PD_HIP(hipGetLastError());
    if (obs) return pd_observe(e, obs, stream);
    return PD_OK;
}

pd_status pd_step(pd_env* e, const void* actions, void* obs, void* reward, uint8_t* done, uint8_t* truncated,
                  int8_t* trunc_id, const double* noise, void* info, void* stream) {
    if (!e || !actions) return fail(PD_ERR_INVALID, "null env/actions");
    PD_HIP(hipSetDevice(e->device));
    StepOut o;
    o.obs = obs; o.reward = reward; o.done = done; o.trunc = truncated; o.tid = trunc_id; o.info = info;
    return with_real(e, [&](auto r) { return step_impl<decltype(r)>(e, actions, o, (hipStream_t)stream, 1, noise); });
}

pd_status pd_step_sac(pd_env* e, const float* mean, const float* log_std, int32_t head_stride, const float* eps,
                      float log_std_min, float log_std_max, float max_action, float* action, float* slab, float* obs32,
                      void* stream) {
    if (!e || !mean) return fail(PD_ERR_INVALID, "null env/mean");
    if (head_stride != 0 && head_stride < e->act_dim) return fail(PD_ERR_INVALID, "pd_step_sac: head_stride < action dim");
    if (eps && !log_std) return fail(PD_ERR_INVALID, "pd_step_sac: eps given without log_std");
    if (e->cfg.action_f64) return fail(PD_ERR_UNSUPPORTED, "pd_step_sac: float32 actions only (action_f64 = 0)");
    if (e->cfg.rtd == PD_RTD_PSO || e->cfg.integrator != PD_INTEG_REFERENCE ||
        (e->cfg.phase != PD_PHASE_PURE_THROTTLE && e->cfg.phase != PD_PHASE_LANDING_BURN))
        return fail(PD_ERR_UNSUPPORTED, "pd_step_sac: the RL landing burns (reference integrator) only");
    PD_HIP(hipSetDevice(e->device));
    const SacIO io{mean, log_std, eps, log_std_min, log_std_max, max_action, action, slab, obs32,
                   (uint32_t)(head_stride ? head_stride : e->act_dim)};
    return sac_step(e, io, stream);
}

pd_status pd_step_sac_ring(pd_env* e, const float* heads, int32_t deterministic, float log_std_min, float log_std_max,
                           float max_action, float* eps_out, float* action, float* ring, int64_t capacity,
                           long long* ring_state, float* priorities, const float* max_priority, float* obs32,
                           void* stream) {
    if (!e || !heads) return fail(PD_ERR_INVALID, "null env/heads");
    if (e->cfg.action_f64) return fail(PD_ERR_UNSUPPORTED, "pd_step_sac_ring: float32 actions only (action_f64 = 0)");
    if (e->cfg.rtd == PD_RTD_PSO || e->cfg.integrator != PD_INTEG_REFERENCE ||
        (e->cfg.phase != PD_PHASE_PURE_THROTTLE && e->cfg.phase != PD_PHASE_LANDING_BURN))
        return fail(PD_ERR_UNSUPPORTED, "pd_step_sac_ring: the RL landing burns (reference integrator) only");
    const int64_t N = e->cfg.n_envs;
    const int64_t W = 2 * (int64_t)e->obs_dim + e->act_dim + 2;
    if (ring_state) {
        if (!ring || capacity < N) return fail(PD_ERR_INVALID, "pd_step_sac_ring: ring mode needs ring and capacity >= n_envs");
        if (capacity * W >= (1ll << 32)) return fail(PD_ERR_INVALID, "pd_step_sac_ring: capacity x row width must be below 2^32");
        if (priorities && !max_priority) return fail(PD_ERR_INVALID, "pd_step_sac_ring: priorities without max_priority");
    }
    PD_HIP(hipSetDevice(e->device));
    const int A = e->act_dim;
    SacIO io{heads, heads + A, nullptr, log_std_min, log_std_max, max_action, action, ring, obs32, (uint32_t)(2 * A)};
    io.draw = deterministic ? 0 : 1;
    io.eps_out = deterministic ? nullptr : eps_out;
    io.ring_cap = ring_state ? capacity : 0;
    io.ring_state = ring_state;
    io.prio = ring_state ? priorities : nullptr;
    io.max_prio = max_priority;
    return sac_step(e, io, stream);
}

pd_status pd_step_sac_fused(pd_env* e, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t n_hidden_layers,
                            const float* const* params, float* heads, int32_t deterministic, float log_std_min,
                            float log_std_max, float max_action, float* eps_out, float* action, float* ring,
                            int64_t capacity, long long* ring_state, float* priorities, const float* max_priority,
                            float* obs32, void* stream) {
    if (!e || !params || !obs32) return fail(PD_ERR_INVALID, "pd_step_sac_fused: null env/params/obs32");
    const int S = e->obs_dim, A = e->act_dim;
    // the actor's widths must be the handle's: its weights are read with the handle's row strides
    if (state_dim != S || action_dim != A)
        return fail(PD_ERR_INVALID, "pd_step_sac_fused: the actor's state_dim / action_dim differ from the handle's");
    if (n_hidden_layers < 1 || n_hidden_layers > kSacMaxLayers || A > 8 || S > 16)
        return fail(PD_ERR_INVALID, "pd_step_sac_fused: 1..8 hidden layers, state_dim <= 16, action_dim <= 8");
    if (hidden != 128 && hidden != 256 && hidden != 512)
        return fail(PD_ERR_UNSUPPORTED, "pd_step_sac_fused: hidden width 128, 256 or 512 only");
    for (int k = 0; k < 2 * (n_hidden_layers + 2); ++k) {
        if (!params[k]) return fail(PD_ERR_INVALID, "pd_step_sac_fused: null parameter");
        if ((uintptr_t)params[k] % 16 != 0) return fail(PD_ERR_UNSUPPORTED, "pd_step_sac_fused: parameter not 16-byte aligned");
    }
    // one launch where the workgroup's envs are one MLP tile (16 lanes per env) and the tile's
    // activations fit the kernel's LDS (hidden <= 256); else pd_sac_actor into `heads` (or the
    // handle's scratch rows) and pd_step_sac_ring: two launches, the same heads bit for bit
    if (e->lpe != 16 || hidden > 256) {
        const int64_t N = e->cfg.n_envs;
        float* h = heads;
        if (!h) {
            if (!e->sac_heads) {
                PD_HIP(hipSetDevice(e->device));
                PD_HIP(hipMalloc((void**)&e->sac_heads, (size_t)N * 2 * A * sizeof(float)));
                e->allocs.push_back(e->sac_heads);
            }
            h = e->sac_heads;
        }
        PD_HIP(hipSetDevice(e->device));
        const pd_status st = pd_sac_actor(N, S, hidden, n_hidden_layers, A, obs32, params, h, stream);
        if (st != PD_OK) return st;
        return pd_step_sac_ring(e, h, deterministic, log_std_min, log_std_max, max_action, eps_out, action, ring,
                                capacity, ring_state, priorities, max_priority, obs32, stream);
    }
    if (e->cfg.action_f64) return fail(PD_ERR_UNSUPPORTED, "pd_step_sac_fused: float32 actions only (action_f64 = 0)");
    if (e->cfg.rtd == PD_RTD_PSO || e->cfg.integrator != PD_INTEG_REFERENCE ||
        (e->cfg.phase != PD_PHASE_PURE_THROTTLE && e->cfg.phase != PD_PHASE_LANDING_BURN))
        return fail(PD_ERR_UNSUPPORTED, "pd_step_sac_fused: the RL landing burns (reference integrator) only");
    const int64_t N = e->cfg.n_envs;
    const int64_t W = 2 * (int64_t)S + A + 2;
    if (ring_state) {
        if (!ring || capacity < N) return fail(PD_ERR_INVALID, "pd_step_sac_fused: ring mode needs ring and capacity >= n_envs");
        if (capacity * W >= (1ll << 32)) return fail(PD_ERR_INVALID, "pd_step_sac_fused: capacity x row width must be below 2^32");
        if (priorities && !max_priority) return fail(PD_ERR_INVALID, "pd_step_sac_fused: priorities without max_priority");
    }
    PD_HIP(hipSetDevice(e->device));
    SacIO io{nullptr, nullptr, nullptr, log_std_min, log_std_max, max_action, action, ring, obs32, (uint32_t)(2 * A)};
    io.draw = deterministic ? 0 : 1;
    io.eps_out = deterministic ? nullptr : eps_out;
    io.ring_cap = ring_state ? capacity : 0;
    io.ring_state = ring_state;
    io.prio = ring_state ? priorities : nullptr;
    io.max_prio = max_priority;
    io.mlp.S = S; io.mlp.L = n_hidden_layers; io.mlp.A = A; io.mlp.H = hidden; io.mlp.obs = obs32;
    for (int l = 0; l < n_hidden_layers; ++l) { io.mlp.w[l] = params[2 * l]; io.mlp.b[l] = params[2 * l + 1]; }
    io.mlp.wm = params[2 * n_hidden_layers]; io.mlp.bm = params[2 * n_hidden_layers + 1];
    io.mlp.ws = params[2 * n_hidden_layers + 2]; io.mlp.bs = params[2 * n_hidden_layers + 3];
    io.heads_out = heads;
    return sac_step(e, io, stream);
}

// The checks pd_rollout_sac and pd_collect_sac share (fn: the entry point's name, what: its kernel):
// an actor the loop kernels' tile holds, on a handle they are instantiated for
static pd_status sac_loop_check(const pd_env* e, const std::string& fn, const std::string& what, int32_t state_dim,
                                int32_t action_dim, int32_t hidden, int32_t n_hidden_layers, const float* const* params) {
    const int S = e->obs_dim, A = e->act_dim;
    if (state_dim != S || action_dim != A)
        return fail(PD_ERR_INVALID, fn + ": the actor's state_dim / action_dim differ from the handle's");
    if (n_hidden_layers < 1 || n_hidden_layers > kSacMaxLayers || A > 8 || S > 16)
        return fail(PD_ERR_INVALID, fn + ": 1..8 hidden layers, state_dim <= 16, action_dim <= 8");
    if (hidden == 512)
        return fail(PD_ERR_UNSUPPORTED, fn + ": hidden width 512 does not fit the " + what + " kernel's LDS tile "
                                        "(128 or 256; use the per-step path, pd_step_sac_fused)");
    if (hidden != 128 && hidden != 256) return fail(PD_ERR_UNSUPPORTED, fn + ": hidden width 128 or 256 only");
    for (int k = 0; k < 2 * (n_hidden_layers + 2); ++k) {
        if (!params[k]) return fail(PD_ERR_INVALID, fn + ": null parameter");
        if ((uintptr_t)params[k] % 16 != 0) return fail(PD_ERR_UNSUPPORTED, fn + ": parameter not 16-byte aligned");
    }
    if (e->cfg.action_f64) return fail(PD_ERR_UNSUPPORTED, fn + ": float32 actions only (action_f64 = 0)");
    if (e->cfg.rtd == PD_RTD_PSO || e->cfg.integrator != PD_INTEG_REFERENCE ||
        (e->cfg.phase != PD_PHASE_PURE_THROTTLE && e->cfg.phase != PD_PHASE_LANDING_BURN))
        return fail(PD_ERR_UNSUPPORTED, fn + ": the RL landing burns (reference integrator) only");
    if (e->lpe != 16)
        return fail(PD_ERR_UNSUPPORTED, fn + ": the handle does not step 16 lanes per env (the workgroup's 16 "
                                        "envs are the actor's MLP tile; use the per-step path, pd_step_sac_fused)");
    return PD_OK;
}

pd_status pd_rollout_sac(pd_env* e, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t n_hidden_layers,
                         const float* const* params, int32_t deterministic, float log_std_min, float log_std_max,
                         float max_action, int32_t reset_first, int32_t max_steps, void* ret, int32_t* steps,
                         uint8_t* done, int8_t* trunc_id, float* actions_out, void* rewards_out, void* stream) {
    if (!e || !params) return fail(PD_ERR_INVALID, "pd_rollout_sac: null env/params");
    if (max_steps < 0) return fail(PD_ERR_INVALID, "pd_rollout_sac: max_steps < 0");
    const int S = e->obs_dim, A = e->act_dim;
    if (const pd_status st = sac_loop_check(e, "pd_rollout_sac", "rollout", state_dim, action_dim, hidden, n_hidden_layers, params))
        return st;
    // the traces are addressed as row base + a 32-bit per-lane byte offset within the row
    if ((uint64_t)e->cfg.n_envs * (uint64_t)A * 4ull >= (1ull << 32))
        return fail(PD_ERR_INVALID, "pd_rollout_sac: n_envs x action_dim x 4 must be below 2^32 bytes");
    PD_HIP(hipSetDevice(e->device));
    SacIO io{nullptr, nullptr, nullptr, log_std_min, log_std_max, max_action, nullptr, nullptr, nullptr, (uint32_t)(2 * A)};
    io.draw = deterministic ? 0 : 1;
    io.mlp.S = S; io.mlp.L = n_hidden_layers; io.mlp.A = A; io.mlp.H = hidden; io.mlp.obs = nullptr;
    for (int l = 0; l < n_hidden_layers; ++l) { io.mlp.w[l] = params[2 * l]; io.mlp.b[l] = params[2 * l + 1]; }
    io.mlp.wm = params[2 * n_hidden_layers]; io.mlp.bm = params[2 * n_hidden_layers + 1];
    io.mlp.ws = params[2 * n_hidden_layers + 2]; io.mlp.bs = params[2 * n_hidden_layers + 3];
    return with_real(e, [&](auto r) {
        return rollout_sac_impl<decltype(r)>(e, io, reset_first, max_steps, ret, steps, done, trunc_id, actions_out,
                                             rewards_out, (hipStream_t)stream);
    });
}

pd_status pd_collect_sac(pd_env* e, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t n_hidden_layers,
                         const float* const* params, int32_t deterministic, float log_std_min, float log_std_max,
                         float max_action, int32_t n_steps, float* ring, int64_t capacity, long long* ring_state,
                         float* priorities, const float* max_priority, float* obs32, float* eps_out, void* reward,
                         uint8_t* done, uint8_t* truncated, int8_t* trunc_id, void* stream) {
    if (!e || !params) return fail(PD_ERR_INVALID, "pd_collect_sac: null env/params");
    if (n_steps < 0) return fail(PD_ERR_INVALID, "pd_collect_sac: n_steps < 0");
    const int S = e->obs_dim, A = e->act_dim;
    if (const pd_status st = sac_loop_check(e, "pd_collect_sac", "collection", state_dim, action_dim, hidden, n_hidden_layers, params))
        return st;
    if (n_steps == 0) return PD_OK;   // (nothing to write: ring and the outputs are not looked at)
    const int64_t N = e->cfg.n_envs;
    const int64_t W = 2 * (int64_t)S + A + 2;
    if (!ring) return fail(PD_ERR_INVALID, "pd_collect_sac: null ring");
    if (ring_state) {
        // (the rows of one launch must not alias -- its workgroups run at different steps -- and
        // position + t N + i stays below 2 capacity: one subtraction wraps it)
        if ((int64_t)n_steps * N > capacity)
            return fail(PD_ERR_INVALID, "pd_collect_sac: ring mode needs capacity >= n_steps x n_envs");
        if (capacity * W >= (1ll << 32)) return fail(PD_ERR_INVALID, "pd_collect_sac: capacity x row width must be below 2^32");
        if (priorities && !max_priority) return fail(PD_ERR_INVALID, "pd_collect_sac: priorities without max_priority");
    } else if ((int64_t)n_steps * N * W >= (1ll << 32)) {
        return fail(PD_ERR_INVALID, "pd_collect_sac: n_steps x n_envs x row width must be below 2^32");
    }
    // eps_out rows are addressed as row base + a 32-bit per-lane byte offset within the row
    if ((uint64_t)N * (uint64_t)A * 4ull >= (1ull << 32))
        return fail(PD_ERR_INVALID, "pd_collect_sac: n_envs x action_dim x 4 must be below 2^32 bytes");
    PD_HIP(hipSetDevice(e->device));
    SacIO io{nullptr, nullptr, nullptr, log_std_min, log_std_max, max_action, nullptr, ring, obs32, (uint32_t)(2 * A)};
    io.draw = deterministic ? 0 : 1;
    io.eps_out = deterministic ? nullptr : eps_out;
    io.ring_cap = ring_state ? capacity : 0;
    io.ring_state = ring_state;
    io.prio = ring_state ? priorities : nullptr;
    io.max_prio = max_priority;
    io.mlp.S = S; io.mlp.L = n_hidden_layers; io.mlp.A = A; io.mlp.H = hidden; io.mlp.obs = nullptr;
    for (int l = 0; l < n_hidden_layers; ++l) { io.mlp.w[l] = params[2 * l]; io.mlp.b[l] = params[2 * l + 1]; }
    io.mlp.wm = params[2 * n_hidden_layers]; io.mlp.bm = params[2 * n_hidden_layers + 1];
    io.mlp.ws = params[2 * n_hidden_layers + 2]; io.mlp.bs = params[2 * n_hidden_layers + 3];
    return with_real(e, [&](auto r) {
        return collect_sac_impl<decltype(r)>(e, io, n_steps, reward, done, truncated, trunc_id, (hipStream_t)stream);
    });
}

pd_status pd_step_n(pd_env* e, const void* actions, int32_t n_steps, void* obs, void* reward, uint8_t* done,
                    uint8_t* truncated, int8_t* trunc_id, void* stream) {
    if (!e || !actions || n_steps < 0) return fail(PD_ERR_INVALID, "bad step_n args");
    if (e->cfg.phase != PD_PHASE_PURE_THROTTLE && e->cfg.phase != PD_PHASE_LANDING_BURN)
        return fail(PD_ERR_UNSUPPORTED, "pd_step_n: landing-burn phases only (use pd_step)");
    PD_HIP(hipSetDevice(e->device));
    return step_n_impl(e, actions, n_steps, obs, reward, done, truncated, trunc_id, nullptr, (hipStream_t)stream);
}

pd_status pd_step_n_info(pd_env* e, const void* actions, int32_t n_steps, void* obs, void* reward, uint8_t* done,
                         uint8_t* truncated, int8_t* trunc_id, void* info, uint64_t info_mask, void* stream) {
    if (!e || !actions || n_steps < 0) return fail(PD_ERR_INVALID, "bad step_n_info args");
    if (e->cfg.phase != PD_PHASE_PURE_THROTTLE && e->cfg.phase != PD_PHASE_LANDING_BURN)
        return fail(PD_ERR_UNSUPPORTED, "pd_step_n_info: landing-burn phases only (use pd_step)");
    if (info && (info_mask == 0 || (info_mask >> PD_N_INFO) != 0))
        return fail(PD_ERR_INVALID, "pd_step_n_info: info_mask must select 1..PD_N_INFO fields of pd_info_field");
    PD_HIP(hipSetDevice(e->device));
    return step_n_impl(e, actions, n_steps, obs, reward, done, truncated, trunc_id, nullptr, (hipStream_t)stream,
                       info, info ? info_mask : 0);
}

pd_status pd_rollout(pd_env* e, const void* actions, int32_t n_steps, void* reward_sum, void* stream) {
    if (!e || !actions || n_steps < 0) return fail(PD_ERR_INVALID, "bad rollout args");
    PD_HIP(hipSetDevice(e->device));
    if (e->cfg.phase == PD_PHASE_PURE_THROTTLE || e->cfg.phase == PD_PHASE_LANDING_BURN)
        return step_n_impl(e, actions, n_steps, nullptr, nullptr, nullptr, nullptr, nullptr, reward_sum,
                           (hipStream_t)stream);
    size_t stride = (size_t)e->cfg.n_envs * e->act_dim * (e->cfg.action_f64 ? 8 : 4);
    StepOut o;
    o.reward_sum = reward_sum;
    for (int32_t t = 0; t < n_steps; ++t) {
        const void* at = (const char*)actions + stride * t;
        pd_status st = with_real(e, [&](auto r) { return step_impl<decltype(r)>(e, at, o, (hipStream_t)stream); });
        if (st != PD_OK) return st;
    }
    return PD_OK;
}

extern "C++" {
namespace {
pd_status rollout_policy_entry(pd_env* e, const float* weights, int32_t n_params, int32_t max_steps, void* fitness,
                               int32_t* steps, int32_t check_every, void* stream, bool chunked) {
    if (!e || !weights || !fitness || max_steps < 0) return fail(PD_ERR_INVALID, "bad policy rollout args");
    if (e->cfg.rtd != PD_RTD_PSO) return fail(PD_ERR_UNSUPPORTED, "policy rollouts need rtd = PD_RTD_PSO");
    if (e->cfg.integrator != PD_INTEG_REFERENCE) return fail(PD_ERR_UNSUPPORTED, "policy rollouts use the reference integrator");
    int want = e->cfg.phase == PD_PHASE_PURE_THROTTLE ? PD_ACTOR_PARAMS_PURE_THROTTLE : PD_ACTOR_PARAMS_LANDING_BURN;
    if (n_params != want) return fail(PD_ERR_INVALID, "n_params does not match the phase's actor");
    if (chunked && (uintptr_t)weights % 16 != 0) return fail(PD_ERR_INVALID, "chunked policy weights must be 16-byte aligned");
    // the kernel addresses the chunked weights [ceil(P/4)][N][4] with 32-bit per-lane byte offsets
    if ((uint64_t)e->cfg.n_envs * (uint64_t)((n_params + 3) / 4) * 16ull >= (1ull << 32))
        return fail(PD_ERR_INVALID, "policy rollouts: n_envs x ceil(n_params / 4) x 16 must be below 2^32 bytes");
    PD_HIP(hipSetDevice(e->device));
    return with_real(e, [&](auto r) {
        return rollout_policy_impl<decltype(r)>(e, weights, max_steps, fitness, steps, check_every, (hipStream_t)stream, chunked);
    });
}
}  // namespace
}  // extern "C++"

pd_status pd_rollout_policy(pd_env* e, const float* weights, int32_t n_params, int32_t max_steps, void* fitness,
                            int32_t* steps, int32_t check_every, void* stream) {
    return rollout_policy_entry(e, weights, n_params, max_steps, fitness, steps, check_every, stream, false);
}

pd_status pd_rollout_policy_chunked(pd_env* e, const float* weights4, int32_t n_params, int32_t max_steps,
                                    void* fitness, int32_t* steps, int32_t check_every, void* stream) {
    return rollout_policy_entry(e, weights4, n_params, max_steps, fitness, steps, check_every, stream, true);
}

pd_status pd_flush_misses(pd_env* e, void* stream) {
    if (!e) return fail(PD_ERR_INVALID, "null env");
    PD_HIP(hipSetDevice(e->device));
    with_real(e, [&](auto r) { launch_insert<decltype(r)>(e, (hipStream_t)stream); });
    PD_HIP(hipGetLastError());
    return PD_OK;
}

pd_status pd_observe(pd_env* e, void* obs, void* stream) {
    if (!e || !obs) return fail(PD_ERR_INVALID, "null env/obs");
    PD_HIP(hipSetDevice(e->device));
    int kind = e->obs_kind;
    unsigned grid = (unsigned)((e->cfg.n_envs + kBlock - 1) / kBlock);
    hipStream_t s = (hipStream_t)stream;
    with_real(e, [&](auto r) {
        using R = decltype(r);
        auto a = make_args<R>(e);
        a.obs = (R*)obs;
        hipLaunchKernelGGL(k_observe<R>, dim3(grid), dim3(kBlock), 0, s, a, kind);
    });
    PD_HIP(hipGetLastError());
    return PD_OK;
}

pd_status pd_get_state(pd_env* e, void* state, void* stream) {
    if (!e || !state) return fail(PD_ERR_INVALID, "null env/state");
    PD_HIP(hipSetDevice(e->device));
    PD_HIP(hipMemcpyAsync(state, e->st, 11 * e->cfg.n_envs * e->rsize, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PD_OK;
}

pd_status pd_set_state(pd_env* e, const void* state, void* stream) {
    if (!e || !state) return fail(PD_ERR_INVALID, "null env/state");
    PD_HIP(hipSetDevice(e->device));
    PD_HIP(hipMemcpyAsync(e->st, state, 11 * e->cfg.n_envs * e->rsize, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PD_OK;
}

pd_status pd_get_actuators(pd_env* e, void* act, void* stream) {
    if (!e || !act) return fail(PD_ERR_INVALID, "null env/act");
    PD_HIP(hipSetDevice(e->device));
    PD_HIP(hipMemcpyAsync(act, e->act, 3 * e->cfg.n_envs * e->rsize, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PD_OK;
}

pd_status pd_set_actuators(pd_env* e, const void* act, void* stream) {
    if (!e || !act) return fail(PD_ERR_INVALID, "null env/act");
    PD_HIP(hipSetDevice(e->device));
    PD_HIP(hipMemcpyAsync(e->act, act, 3 * e->cfg.n_envs * e->rsize, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PD_OK;
}

pd_status pd_set_gload_window(pd_env* e, const void* vprev, const void* window, const uint8_t* len, void* stream) {
    if (!e || !vprev || !window || !len) return fail(PD_ERR_INVALID, "null env/vprev/window/len");
    PD_HIP(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)e->cfg.n_envs;
    PD_HIP(hipMemcpyAsync(e->vprev, vprev, N * e->rsize, hipMemcpyDeviceToDevice, s));
    PD_HIP(hipMemcpyAsync(e->gwin, window, 10 * N * e->rsize, hipMemcpyDeviceToDevice, s));
    PD_HIP(hipMemcpyAsync(e->glen, len, N, hipMemcpyDeviceToDevice, s));
    PD_HIP(hipMemsetAsync(e->ghead, 0, N, s));   // oldest entry in slot 0
    return PD_OK;
}

pd_status pd_set_wind_sigmas(pd_env* e, const double* sig, void* stream) {
    if (!e || !sig) return fail(PD_ERR_INVALID, "null env/sig");
    PD_HIP(hipSetDevice(e->device));
    unsigned grid = (unsigned)((e->cfg.n_envs + kBlock - 1) / kBlock);
    hipStream_t s = (hipStream_t)stream;
    with_real(e, [&](auto r) { using R = decltype(r); hipLaunchKernelGGL(k_set_sigmas<R>, dim3(grid), dim3(kBlock), 0, s, make_args<R>(e), sig); });
    PD_HIP(hipGetLastError());
    return PD_OK;
}

pd_status pd_counters(pd_env* e, int64_t* misses, int64_t* ecd, int64_t* ecl, int64_t* nans) {
    if (!e) return fail(PD_ERR_INVALID, "null env");
    PD_HIP(hipSetDevice(e->device));
    unsigned long long st[kStats];
    PD_HIP(hipMemcpy(st, e->pend.stats, sizeof(st), hipMemcpyDeviceToHost));
    if (misses) *misses = (int64_t)st[0];
    if (nans) *nans = (int64_t)st[1];
    if (ecd) *ecd = (int64_t)st[2];
    if (ecl) *ecl = (int64_t)st[3];
    return PD_OK;
}

pd_status pd_atmosphere(pd_env* e, const void* altitude, void* out, int64_t n, void* stream) {
    if (!e || !altitude || !out || n < 0) return fail(PD_ERR_INVALID, "bad pd_atmosphere args");
    if (n == 0) return PD_OK;
    PD_HIP(hipSetDevice(e->device));
    unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
    hipStream_t s = (hipStream_t)stream;
    with_real(e, [&](auto r) {
        using R = decltype(r);
        hipLaunchKernelGGL(k_atmosphere<R>, dim3(grid), dim3(kBlock), 0, s, make_args<R>(e), (const R*)altitude, (R*)out, n);
    });
    PD_HIP(hipGetLastError());
    return PD_OK;
}

pd_status pd_stats(pd_env* e, int64_t* out, int32_t n) {
    if (!e || !out || n < 0) return fail(PD_ERR_INVALID, "bad pd_stats args");
    PD_HIP(hipSetDevice(e->device));
    unsigned long long st[kStats];
    PD_HIP(hipMemcpy(st, e->pend.stats, sizeof(st), hipMemcpyDeviceToHost));
    for (int32_t k = 0; k < n && k < kStats; ++k) out[k] = (int64_t)st[k];
    return PD_OK;
}

pd_status pd_count_work(pd_env* e, int32_t enable) {
    if (!e) return fail(PD_ERR_INVALID, "null env");
    e->count_work = enable != 0;
    return PD_OK;
}

pd_status pd_get_gload_window(pd_env* e, void* vprev, void* window, uint8_t* len, uint8_t* head, void* stream) {
    if (!e) return fail(PD_ERR_INVALID, "null env");
    PD_HIP(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)e->cfg.n_envs;
    if (vprev) PD_HIP(hipMemcpyAsync(vprev, e->vprev, N * e->rsize, hipMemcpyDeviceToDevice, s));
    if (window) PD_HIP(hipMemcpyAsync(window, e->gwin, 10 * N * e->rsize, hipMemcpyDeviceToDevice, s));
    if (len) PD_HIP(hipMemcpyAsync(len, e->glen, N, hipMemcpyDeviceToDevice, s));
    if (head) PD_HIP(hipMemcpyAsync(head, e->ghead, N, hipMemcpyDeviceToDevice, s));
    return PD_OK;
}

pd_status pd_get_wind_state(pd_env* e, void* filters, void* sigmas, uint8_t* profile, void* stream) {
    if (!e) return fail(PD_ERR_INVALID, "null env");
    PD_HIP(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)e->cfg.n_envs;
    if (filters) PD_HIP(hipMemcpyAsync(filters, e->wind, 4 * N * e->rsize, hipMemcpyDeviceToDevice, s));
    if (sigmas) PD_HIP(hipMemcpyAsync(sigmas, (char*)e->wind + 4 * N * e->rsize, 2 * N * e->rsize, hipMemcpyDeviceToDevice, s));
    if (profile) PD_HIP(hipMemcpyAsync(profile, e->wprof, N, hipMemcpyDeviceToDevice, s));
    return PD_OK;
}

// The wind profile bytes of n envs (device memory) are all valid ids (percentile - 50 in 0..49):
// k_step indexes the LDS profiles and wind_n[] with them.  Stream-ordered read-back (setters only).
static pd_status check_profiles(const uint8_t* dev, size_t n, hipStream_t s) {
    std::vector<uint8_t> h(n);
    PD_HIP(hipMemcpyAsync(h.data(), dev, n, hipMemcpyDeviceToHost, s));
    PD_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i)
        if (h[i] >= PD_N_WIND_PROFILES)
            return fail(PD_ERR_INVALID, "wind profile id " + std::to_string(h[i]) + " of env " + std::to_string(i) +
                                            " out of range (percentile must be 50..99)");
    return PD_OK;
}

pd_status pd_set_wind_state(pd_env* e, const void* filters, const void* sigmas, const uint8_t* profile, void* stream) {
    if (!e) return fail(PD_ERR_INVALID, "null env");
    PD_HIP(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)e->cfg.n_envs;
    if (profile) {   // refused before anything is written
        pd_status st = check_profiles(profile, N, s);
        if (st != PD_OK) return st;
    }
    if (filters) PD_HIP(hipMemcpyAsync(e->wind, filters, 4 * N * e->rsize, hipMemcpyDeviceToDevice, s));
    if (sigmas) PD_HIP(hipMemcpyAsync((char*)e->wind + 4 * N * e->rsize, sigmas, 2 * N * e->rsize, hipMemcpyDeviceToDevice, s));
    if (profile) PD_HIP(hipMemcpyAsync(e->wprof, profile, N, hipMemcpyDeviceToDevice, s));
    return PD_OK;
}

pd_status pd_get_counters(pd_env* e, uint32_t* episode, uint32_t* step, int8_t* trunc_id, void* stream) {
    if (!e) return fail(PD_ERR_INVALID, "null env");
    PD_HIP(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)e->cfg.n_envs;
    if (episode) PD_HIP(hipMemcpyAsync(episode, e->epi, N * 4, hipMemcpyDeviceToDevice, s));
    if (step) PD_HIP(hipMemcpyAsync(step, e->tstep, N * 4, hipMemcpyDeviceToDevice, s));
    if (trunc_id) PD_HIP(hipMemcpyAsync(trunc_id, e->tid, N, hipMemcpyDeviceToDevice, s));
    return PD_OK;
}

pd_status pd_set_counters(pd_env* e, const uint32_t* episode, const uint32_t* step, const int8_t* trunc_id,
                          void* stream) {
    if (!e) return fail(PD_ERR_INVALID, "null env");
    PD_HIP(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)e->cfg.n_envs;
    if (episode) PD_HIP(hipMemcpyAsync(e->epi, episode, N * 4, hipMemcpyDeviceToDevice, s));
    if (step) PD_HIP(hipMemcpyAsync(e->tstep, step, N * 4, hipMemcpyDeviceToDevice, s));
    if (trunc_id) PD_HIP(hipMemcpyAsync(e->tid, trunc_id, N, hipMemcpyDeviceToDevice, s));
    return PD_OK;
}

// The per-env buffers of a handle in checkpoint-blob order, each 16-byte aligned in the blob.
static int checkpoint_fields(const pd_env* e, void** ptr, size_t* bytes) {
    const size_t N = (size_t)e->cfg.n_envs, R = e->rsize;
    void* p[] = {e->st, e->vprev, e->gwin, e->act, e->wind, e->ghead, e->glen, e->wprof, e->key, e->slot,
                 e->tid, e->epi, e->tstep, e->fin};
    size_t b[] = {11 * N * R, N * R, 10 * N * R, 3 * N * R, 6 * N * R, N, N, N, 2 * N * 8, 2 * N * 4, N, N * 4, N * 4, N};
    const int n = (int)(sizeof(b) / sizeof(b[0]));
    for (int k = 0; k < n; ++k) { ptr[k] = p[k]; bytes[k] = b[k]; }
    return n;
}
static size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

size_t pd_checkpoint_size(const pd_env* e) {
    if (!e) return 0;
    void* p[16]; size_t b[16];
    int n = checkpoint_fields(e, p, b);
    size_t t = 0;
    for (int k = 0; k < n; ++k) t += align16(b[k]);
    return t;
}

pd_status pd_checkpoint_save(pd_env* e, void* blob, void* stream) {
    if (!e || !blob) return fail(PD_ERR_INVALID, "null env/blob");
    PD_HIP(hipSetDevice(e->device));
    void* p[16]; size_t b[16];
    int n = checkpoint_fields(e, p, b);
    size_t off = 0;
    for (int k = 0; k < n; ++k) {
        PD_HIP(hipMemcpyAsync((char*)blob + off, p[k], b[k], hipMemcpyDeviceToDevice, (hipStream_t)stream));
        off += align16(b[k]);
    }
    return PD_OK;
}

pd_status pd_checkpoint_load(pd_env* e, const void* blob, void* stream) {
    if (!e || !blob) return fail(PD_ERR_INVALID, "null env/blob");
    PD_HIP(hipSetDevice(e->device));
    void* p[16]; size_t b[16];
    int n = checkpoint_fields(e, p, b);
    size_t off = 0;
    for (int k = 0; k < n; ++k) {   // a blob with invalid wind profile ids is refused before loading
        if (p[k] == e->wprof) {
            pd_status st = check_profiles((const uint8_t*)blob + off, b[k], (hipStream_t)stream);
            if (st != PD_OK) return st;
        }
        off += align16(b[k]);
    }
    off = 0;
    for (int k = 0; k < n; ++k) {
        PD_HIP(hipMemcpyAsync(p[k], (const char*)blob + off, b[k], hipMemcpyDeviceToDevice, (hipStream_t)stream));
        off += align16(b[k]);
    }
    return PD_OK;
}

int pd_obs_dim(const pd_env* e) { return e ? e->obs_dim : 0; }
int pd_action_dim(const pd_env* e) { return e ? e->act_dim : 0; }

}  // extern "C"
