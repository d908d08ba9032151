/* pdenv.h -- C ABI of the MI355X-native vectorised powered-descent environment (libpdenv.so).
 *
 * Drop-in boundary for the hot path of JvanZyl1/PSSO-SAC-for-powered-descent.  The reference
 * has no FFI: its seam is the Python object API, which this ABI replaces one-for-one for a
 * batch of N environments living in HBM:
 *
 *   pd_create   <- rocket_environment_pre_wrap.__init__ + compile_physics + compile_rtd_{rl,pso}
 *                  (src/envs/base_environment.py:13-78, src/envs/rockets_physics.py:707-998,
 *                   src/envs/rl/rtd_rl.py:537-604, src/envs/pso/rtd_pso.py:320-383)
 *   pd_reset    <- rocket_environment_pre_wrap.reset (base_environment.py:80-97)
 *   pd_step     <- rocket_environment_pre_wrap.step  (base_environment.py:99-154), i.e.
 *                  physics_step x4 sub-steps (rockets_physics.py:455-704, :857-860, :953-956),
 *                  g-load window, truncated_func -> done_func -> reward_func, plus the wrapper's
 *                  observation (env_wrapped_rl_pytorch.py:167-202 / env_wrapped_ea.py:97-123)
 *   pd_get_state/pd_set_state <- .state attribute (teacher forcing, checkpoint, perturbation)
 *   trunc_id output of pd_step <- rl_wrapped_env_pytorch.truncation_id (env_wrapped_rl_pytorch.py:117-118)
 *   pd_rollout_policy <- pso_wrapped_env.objective_function + simple_actor.forward for a batch of
 *                  particles (env_wrapped_ea.py:18-44, 200-222; particle_swarm_optimisation.py:334-350)
 *
 * Conventions: plain C, no torch types.  All array arguments are DEVICE pointers (HBM) owned by
 * the caller, laid out env-major [N] or [N][k]; `stream` is a hipStream_t (NULL = default).
 * Calls are asynchronous and stream-ordered; a handle is not thread-safe (one per GPU/shard).
 * Floating point buffers use the handle's precision: double for PD_F64, float for PD_F32.
 * Errors are returned as pd_status codes; pd_last_error() gives a thread-local message.
 */
#ifndef PDENV_H
#define PDENV_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PD_ABI_VERSION 11  /* 4: pd_config.integrator (was padding); 5: pd_count_work, pd_step_sac; 6: cell pieces (pd_cell_piece_info, stats word 44); 7: pd_step_sac_ring, pd_sac_actor, stats word 45; 8: pd_step_sac_fused, pd_atm_table; 9: pd_config.table_flags, pd_tuning, caller scratch for pd_pso_swarm_minima, state/action dims of pd_step_sac_fused; 10: step launches insert their own solved misses (pd_flush_misses optional), explicit list settings turn the auto refill off; 11: pd_pso_step_chunked, pd_rollout_policy_chunked; pd_rollout_sac, then pd_atm_table_lds, pd_wind_slopes, PD_TABLES_NO_ATM_LDS and PD_TABLES_NO_PACE added later as additive exports (the version stays 11: no layout or existing call changes) */
#define PD_MAX_PTS 256      /* aero scatter points per table */
#define PD_MAX_COLS 5       /* AoA columns per aero table */
#define PD_MAX_TAB 64       /* grid-fin table length */
#define PD_MAX_WIND 16      /* nodes per wind profile */
#define PD_N_WIND_PROFILES 50   /* integer percentiles 50..99 */
#define PD_N_STATE 11       /* x y vx vy theta theta_dot gamma alpha mass mass_propellant time */
#define PD_N_INFO 49        /* see pd_info_field */
/* simple_actor sizes of the PSO drivers (env_wrapped_ea.py:18-36, 174-185):
 * pure throttle 2-8-(8-8)x3-1, landing_burn 5-8-(8-8)x4-4 */
#define PD_ACTOR_PARAMS_PURE_THROTTLE 249
#define PD_ACTOR_PARAMS_LANDING_BURN 372

typedef enum { PD_OK = 0, PD_ERR_INVALID = 1, PD_ERR_HIP = 2, PD_ERR_NOMEM = 3, PD_ERR_UNSUPPORTED = 4 } pd_status;
/* compile_physics flight phases (rockets_physics.py:707-998; base_environment.py:21).  Actions:
 * 1 (pure throttle: throttle; Pcontrol: v_ref; ballistic: RCS; flip-over: gimbal), 4 (landing_burn),
 * 2 (subsonic/supersonic: gimbal, throttle).  PD_PHASE_LANDING_BURN_ACS is accepted by the
 * enum but pd_create refuses it: the reference raises TypeError at its first step
 * (rockets_physics.py:867-891 calls the gimballed decomposer with ACS arguments;
 * base_environment.py:126-130 passes two prevs to a three-prev lambda). */
typedef enum {
    PD_PHASE_PURE_THROTTLE = 0, PD_PHASE_LANDING_BURN = 1, PD_PHASE_PCONTROL = 2,
    PD_PHASE_BALLISTIC_ARC = 3, PD_PHASE_FLIP_OVER = 4, PD_PHASE_SUBSONIC = 5, PD_PHASE_SUPERSONIC = 6,
    PD_PHASE_LANDING_BURN_ACS = 7
} pd_phase;
/* reward/truncated/done family: rtd_rl.py, rtd_pso.py, or none (compile_physics stepping only:
 * reward 0, never done/truncated).  Pairs the reference cannot step are refused by pd_create
 * with PD_ERR_UNSUPPORTED: RL + flip-over (rtd_rl.py:134 truncated_func takes one argument,
 * base_environment.py:150 passes three), PSO + any phase but the two landing burns (the same
 * arity mismatch in rtd_pso.py:38,107,141). */
typedef enum { PD_RTD_RL = 0, PD_RTD_PSO = 1, PD_RTD_NONE = 2 } pd_rtd;
typedef enum { PD_F64 = 0, PD_F32 = 1 } pd_precision;
/* Integrator of the physics sub-steps.  PD_INTEG_REFERENCE is the reference's semi-implicit Euler
 * (compile_physics, rockets_physics.py:909-957 / 803-861) and the only mode with reference
 * parity.  PD_INTEG_RK4 is NOT the reference: BASELINE config c2's "RK4 dt=0.01 s" (SURVEY 8(d)
 * c2, "benchmarked separately, labelled non-parity"), classical RK4 over (x, y, vx, vy, theta,
 * theta_dot, mass, mass_propellant) with rocket_physics_fcn's forces at every stage, 10 x 0.01 s
 * per 0.1 s env step; landing_burn_pure_throttle without wind only (the von Karman gusts are a
 * discrete-time process), no policy rollouts.  Checked against the oracle's restatement
 * (orc_physics, ORC_INTEG_RK4), not against the reference. */
typedef enum { PD_INTEG_REFERENCE = 0, PD_INTEG_RK4 = 1 } pd_integrator;
/* pd_config.table_flags: how the aero and atmosphere lookups are served (results agree within the
 * tolerances of DESIGN.md s4/s8; the cell-piece, fine-index and carry switches give the same bits as
 * their default, which the GPU tests check).  0 = the defaults. */
typedef enum {
    PD_TABLES_NO_CELL_PIECES = 1,   /* interior C_D/C_L queries by payload sums, not cell pieces */
    PD_TABLES_NO_FINE_INDEX = 2,    /* cell pieces reached through the cell / sub-cell records only */
    PD_TABLES_EXACT_ATMOSPHERE = 4, /* the ISA closed form on the device, never the tabulated pieces */
    PD_TABLES_VERBOSE = 8,          /* print the table builders' statistics to stderr at create */
    PD_TABLES_NO_CARRY = 16,        /* the step kernel's searches take no carried interval as a guess */
    PD_TABLES_NO_ATM_LDS = 32,      /* no coarse atmosphere table in the 512-thread step kernels' LDS: the closed form */
    PD_TABLES_NO_PACE = 64          /* the 512-thread step kernels' waves never change their issue priority (builds with PD_PACE; the same bits either way) */
} pd_table_flags;

/* One neighbourhood-aero table: scatter points grouped by AoA column, Mach-sorted inside. */
typedef struct {
    int32_t n_cols, n_pts;
    double col_aoa[PD_MAX_COLS];
    int32_t col_start[PD_MAX_COLS], col_len[PD_MAX_COLS];
    double mach[PD_MAX_PTS];
    double coef[PD_MAX_PTS];
} pd_aero_table;

/* Physical parameter pack (host memory); filled from data/param_pack.json by the loader. */
typedef struct {
    /* sizing_results.csv (rockets_physics.py:714-719, size_gust_coefficients.py:3-22) */
    double thrust_per_engine, nozzle_exit_pressure, nozzle_exit_area, v_exhaust;
    int32_t n_engines_gimballed, pad0;
    double grid_fin_area, d_base_grid_fin, rocket_radius, frontal_area, m_prop0, C_gust_x, C_gust_y;
    /* stage-2 stage_inertia closure constants (rocket_dimensions.py:158-197) */
    double h_ox, h_f, m_ox, m_f, h_lower, m_dry, x_dry, I_dry, engine_height, cop;
    /* ISA layer table (ambiance) + gravity (atmosphere_dynamics.py:5-33) */
    double isa_Hb[9], isa_Tb[9], isa_beta[9], isa_pb[9];
    double isa_g0, isa_R, isa_kappa, isa_r, isa_alt_max, grav_R, grav_g0;
    /* V2 aero (aerodynamic_coefficients.py:8-66) */
    pd_aero_table cd, cl;
    /* grid fins (grid_fin_aerodynamics.py:7-46), x sorted */
    int32_t ca_n, cn_n;
    double ca_x[PD_MAX_TAB], ca_y[PD_MAX_TAB], ca_min_mach, ca_min_val;
    double cn_x[PD_MAX_TAB], cn_y[PD_MAX_TAB], cn_min_mach, cn_max_mach, cn_min_val, cn_max_val, cn_slope;
    /* wind (HorizontalWindSpeed.py, vonkarman.py): profiles for percentiles 50..99 */
    int32_t wind_n[PD_N_WIND_PROFILES];
    double wind_alt_km[PD_N_WIND_PROFILES][PD_MAX_WIND], wind_speed[PD_N_WIND_PROFILES][PD_MAX_WIND];
    double vk_Ad_u[4], vk_Bd_u[2], vk_Ad_v[4], vk_Bd_v[2], vk_y_threshold;
    double sigma_u_lo, sigma_u_hi, sigma_v_lo, sigma_v_hi;
    /* initial state (load_initial_states.py:236-242) and observation normalisers */
    double state0[PD_N_STATE];
    double norm_y, norm_vy, norm_x, norm_vx;
    /* pre-enumerated neighbourhood keys of the two aero tables (host arrays, may be NULL) */
    const uint64_t* keys_cd; int64_t n_keys_cd;
    const uint64_t* keys_cl; int64_t n_keys_cl;
    /* ---- ABI 2: the other flight phases (rockets_physics.py:17-166,402-451,728-802,959-997) */
    /* full_rocket_inertia cells of x_cog_inertia_subrocket_0_lambda (rocket_dimensions.py:198-241):
     * x_wet_2_initial, x_dry_1, m_s_1, m_pay, m_2, m_1_ox, m_1_f, h_lower_1, h_1_ox, h_1_f, h_1,
     * I_wet_2_initial, I_dry_1 */
    double full_rocket[13];
    double cop_ascent;                  /* cop_func(h_1 + h_2, d_0 = 0.25) (main_sizing.py:215) */
    int32_t n_engines_stage1, pad1;     /* 42: 16 gimballed + 26 fixed in the ascent */
    double rcs_force, rcs_d_bottom, rcs_d_top;   /* RCS (rockets_physics.py:149-166, 784-786) */
    double state0_phase[8][PD_N_STATE]; /* initial state per pd_phase (load_initial_states.py) */
    double norm_phase[8][8];            /* RL observation normalisers (input_normalisation.py) */
    /* ascent reference trajectory sorted by y (reference_trajectory_interpolation.py:5-37) */
    const double* ref_y; const double* ref_x; const double* ref_vx; const double* ref_vy;
    int32_t n_ref, pad2;
    double hyper[2][12][9];             /* rtd_rl.py:543-574, subsonic / supersonic */
    double terminal_mach[2];            /* rtd_rl.py:576-589 */
} pd_params;

typedef struct {
    int64_t n_envs;
    int32_t device;            /* HIP device ordinal */
    int32_t phase;             /* pd_phase */
    int32_t rtd;               /* pd_rtd */
    int32_t precision;         /* pd_precision */
    uint64_t seed;             /* Philox key (wind normals, sigmas, percentiles, tilt) */
    uint64_t env_offset;       /* global index of env 0 (multi-GPU shards draw disjoint streams) */
    int32_t enable_wind, stochastic_wind;
    int32_t wind_percentile;   /* 50..99, or -1 = float(randint(50, 99)) per reset */
    int32_t auto_reset;        /* reset envs in-kernel when done|truncated */
    double tilt_sigma_rad;     /* initial pitch perturbation N(0, s) (0 = reference) */
    int32_t action_f64;        /* actions are double (f64 path, no float32 islands) */
    int32_t lanes_per_env;     /* step-kernel lanes per env: 1, 2, 4, 8 or 16 (0 = by n_envs: 16 up
                                  to 4 096 envs, 8 up to 8 192, 4 up to 16 384, else 2; policy
                                  rollouts use at most 8) */
    /* ---- ABI 2 */
    double dt;                 /* physics dt of phases 2..6, compile_physics(dt, phase) (0 = the env's 0.1) */
    double discount_factor;    /* rtd_rl landing_burn reward scale (1-g)/(1-g^L) and the Pcontrol
                                  alive bonus 0.01 (1-g) (rtd_rl.py:267, 472); rl_wrapped_env_pytorch kwargs */
    int32_t trajectory_length;
    int32_t integrator;        /* pd_integrator (ABI 4; 0 = the reference's) */
    int32_t table_flags;       /* pd_table_flags (ABI 9; 0 = the defaults) */
    int32_t pad3;
} pd_config;

/* Launch tuning of a handle (pd_set_tuning / pd_get_tuning; ABI 9).  Results never depend on it:
 * every setting steps the same envs through the same arithmetic. */
typedef struct {
    int32_t step_fuse;        /* env-steps per pd_step_n / pd_rollout launch, 1..256 (default 128) */
    int32_t policy_fuse;      /* policy steps per pd_rollout_policy launch: a power of two 1..64 (default 64) */
    int32_t policy_lanes;     /* lanes per env of the policy rollouts: 2 (default), 4 or 8 */
    int32_t policy_list;      /* live-list launches of the policy rollouts: -1 = when the grid exceeds
                                 one chip round (default), 0 = never, 1 = from the first launch */
    double policy_list_at;    /* > 0 (with policy_list -1 or 0): switch the list on once the live count
                                 read back falls to this fraction of n_envs (default 0: never) */
    int32_t policy_refill;    /* refill rollouts: -1 = every windless swarm of at least one wave's slots
                                 unless policy_list >= 0 or policy_list_at > 0 asks for the per-check
                                 launches (default; pool batch 3/4 of a wave's slots), 0 = never, k in
                                 1..64 = on (policy_list, policy_list_at and check_every then do nothing),
                                 pool batch k.  One launch of policy_slots env slots (0: the resident
                                 capacity) steps the whole swarm: a wave's slots take the next particles
                                 of its own range as their episodes end (no atomic; policy_refill_own),
                                 then the shared pool's once k of them wait (or none is live: a wave
                                 ballot, one atomic).  Windy handles: the per-check launches */
    int32_t policy_slots;     /* env slots of a refill rollout (0 = the chip's resident capacity; rounded
                                 down to whole waves) */
    int32_t policy_refill_own;/* refill rollouts: percent of the swarm handed out from the waves' own
                                 particle ranges (no atomic), the rest from the shared pool; -1 = 100 */
    int32_t pad_tuning;
} pd_tuning;

/* Info tap of pd_step: the quantities of the LAST physics sub-step that rocket_physics_fcn puts in
 * its info dict (rockets_physics.py:649-702, incl. acceleration_dict / moments_dict), the
 * action_info of the phase's control law and the ACS's acs_info (acs_model.py:62-86), and the
 * env's g_load_1_sec_window (base_environment.py:149).  Layout [PD_N_INFO][N].  Entries that are
 * arithmetic of these and the post-step state (accelerations, gravity_force_y, F_n_L = C_n_L qS,
 * ...) are formed by the caller (pdenv/wrappers.py builds the reference's dict). */
typedef enum {
    PD_INFO_AIR_DENSITY = 0, PD_INFO_PRESSURE, PD_INFO_SPEED_OF_SOUND, PD_INFO_MACH, PD_INFO_Q,
    PD_INFO_CL, PD_INFO_CD, PD_INFO_MASS_FLOW, PD_INFO_X_COG, PD_INFO_INERTIA, PD_INFO_ALPHA_EFF,
    PD_INFO_THROTTLE, PD_INFO_GLOAD, PD_INFO_UG, PD_INFO_VG, PD_INFO_GIMBAL_DEG,
    PD_INFO_MACH_MAX,                  /* sqrt(2 Qmax / rho) / a, Qmax 30000 (200 above the ISA) */
    PD_INFO_DRAG, PD_INFO_LIFT, PD_INFO_D_CP_CG, PD_INFO_D_THRUST_CG, PD_INFO_FUEL_CONSUMED,
    PD_INFO_CF_PAR, PD_INFO_CF_PERP, PD_INFO_CF_X, PD_INFO_CF_Y, PD_INFO_AERO_X, PD_INFO_AERO_Y,
    PD_INFO_GRAVITY,                   /* g at the sub-step's altitude */
    PD_INFO_F_WIND_X, PD_INFO_F_WIND_Y, PD_INFO_VX_DOT, PD_INFO_VY_DOT,
    PD_INFO_CONTROL_MOMENT, PD_INFO_AERO_MOMENT, PD_INFO_M_WIND, PD_INFO_MOMENTS, PD_INFO_THETA_DDOT,
    PD_INFO_DCMD_L, PD_INFO_DCMD_R,    /* fin deflection commands (rad) */
    PD_INFO_DELTA_L, PD_INFO_DELTA_R,  /* filtered fin deflections (rad) */
    PD_INFO_GF_CA, PD_INFO_GF_CN_L, PD_INFO_GF_CN_R,   /* grid-fin C_a, C_n of the left/right fin */
    PD_INFO_GF_F_PERP, PD_INFO_GF_F_PAR, PD_INFO_GF_MZ, /* grid-fin force perpendicular/parallel, moment */
    PD_INFO_THETA_IN                   /* pitch at the start of the sub-step (the ACS's pitch_angle) */
} pd_info_field;

typedef struct pd_env pd_env;

int pd_abi_version(void);
/* sizeof(pd_params) / sizeof(pd_config) as compiled, for binding-layout checks */
size_t pd_sizeof_params(void);
size_t pd_sizeof_config(void);
const char* pd_last_error(void);
/* Number of HIP devices visible (0 without a GPU); never aborts. */
int pd_device_count(void);

pd_status pd_create(const pd_params* params, const pd_config* cfg, pd_env** out);
pd_status pd_destroy(pd_env* env);
/* Launch tuning (see pd_tuning); PD_ERR_INVALID, changing nothing, for out-of-range fields. */
pd_status pd_set_tuning(pd_env* env, const pd_tuning* tuning);
pd_status pd_get_tuning(const pd_env* env, pd_tuning* tuning);
/* Reset envs (mask: device uint8[N], NULL = all).  obs may be NULL. */
pd_status pd_reset(pd_env* env, const uint8_t* mask, void* obs, void* stream);
/* One env step for all N envs.
 *  actions : [N][A] float32 (or double when cfg.action_f64), A = 1 or 4
 *  obs     : [N][O] (O = 2 pure throttle, 5 PSO landing_burn), post-step (pre-auto-reset)
 *  reward  : [N]; done, truncated: uint8 [N]; trunc_id: int8 [N]   (any output may be NULL)
 *  noise   : optional [N][8] double standard normals replacing the Philox wind stream
 *            (sub-step k uses noise[2k], noise[2k+1]; test injection), NULL = Philox
 *  info    : optional [PD_N_INFO][N] (last sub-step values), NULL = not written */
pd_status pd_step(pd_env* env, const void* actions, void* obs, void* reward, uint8_t* done,
                  uint8_t* truncated, int8_t* trunc_id, const double* noise, void* info, void* stream);
/* n_steps consecutive pd_step calls over device-resident actions [n_steps][N][A], landing-burn
 * phases: obs [n_steps][N][O], reward [n_steps][N], done/truncated/trunc_id [n_steps][N] receive
 * every step's outputs (any may be NULL).  Replaces a Python loop over
 * rocket_environment_pre_wrap.step (base_environment.py:99-154) with fused launches: each launch
 * runs up to 128 steps (pd_tuning.step_fuse, 1..256) of every env in one kernel, so the LDS table staging and the
 * launch tail are paid once per launch, followed by the miss flush.  Results are bit-identical
 * to n_steps pd_step calls.  No host synchronisation. */
pd_status pd_step_n(pd_env* env, const void* actions, int32_t n_steps, void* obs, void* reward, uint8_t* done,
                    uint8_t* truncated, int8_t* trunc_id, void* stream);
/* pd_step_n with the info tap in the fused launches (ABI 9): info [n_steps][k][N] (handle
 * precision) receives, for every step, the k = popcount(info_mask) fields of pd_info_field whose
 * bit is set in info_mask, in pd_info_field order -- the visualisation episodes' selected keys
 * (rockets_physics.py:649-702) without a launch per step.  The same values as pd_step's info. */
pd_status pd_step_n_info(pd_env* env, const void* actions, int32_t n_steps, void* obs, void* reward, uint8_t* done,
                         uint8_t* truncated, int8_t* trunc_id, void* info, uint64_t info_mask, void* stream);
/* One SAC data-collection step (sac_pytorch_powered_descent.py:160-183 for N envs) in one
 * launch.  The action is sampled in the kernel from the caller's actor heads, as Actor.sample
 * does it (sac_pytorch.py:161-179) in binary32: a = tanh(mean + exp(clamp(log_std, log_std_min,
 * log_std_max)) * eps) * max_action, or tanh(mean) * max_action when eps is NULL (deterministic);
 * mean, log_std: float32 rows of head_stride floats (0: A), e.g. both heads of one [N][2A] GEMM
 * with log_std = mean + A and head_stride 2A; eps [N][A] float32 standard normals (e.g.
 * torch.randn).  Then the env steps
 * as pd_step (auto-reset per config) and the kernel epilogue writes, all float32 and any of them
 * NULL: action [N][A]; slab [N][2 S + A + 2], the replay buffer's transition row
 * state | action | reward | next_state | done (sac_pytorch.py:27-35; next_state the terminal
 * observation before any reset, done without truncation, as the driver stores them,
 * sac_pytorch_powered_descent.py:170-176); obs32 [N][S], the observation the actor sees next
 * (after any auto-reset).  RL landing-burn handles (PD_PHASE_PURE_THROTTLE / PD_PHASE_LANDING_BURN,
 * rtd RL or NONE, reference integrator) with float32 actions only.  No host synchronisation. */
pd_status pd_step_sac(pd_env* env, const float* mean, const float* log_std, int32_t head_stride, const float* eps,
                      float log_std_min, float log_std_max, float max_action, float* action, float* slab, float* obs32,
                      void* stream);
/* pd_step_sac with the rest of the collection step folded into the same launch (c5):
 *  heads   : [N][2A] float32, mean | log_std as Actor.forward's two heads leave them (unclamped),
 *            e.g. from pd_sac_actor
 *  deterministic != 0: a = tanh(mean) * max_action; else eps ~ N(0, 1) is drawn in the kernel
 *            (torch.randn's role in Normal.rsample, sac_pytorch.py:170-172): Philox4x32-10 keyed
 *            by the handle's seed, counter (env, episode, step, tag 19 + a/2), Box-Muller as the
 *            wind gusts; eps_out [N][A] (may be NULL) receives the draws
 *  ring    : the replay buffer's transition rows [capacity][2S + A + 2] float32 (sac_pytorch.py:
 *            12-49); with ring_state != NULL env i's row goes to (ring_state[0] + i) mod capacity,
 *            priorities[row] = *max_priority (PrioritizedReplayBuffer.add, sac_pytorch.py:76-83;
 *            priorities may be NULL), and the launch's last workgroup sets ring_state[0] (position)
 *            += N mod capacity, ring_state[1] (size) = min(size + N, capacity); ring_state[2] is
 *            its workgroup counter and must be 0 between launches (capacity >= N).  With
 *            ring_state NULL, ring is a [N][2S + A + 2] slab (pd_step_sac's).
 *  action, obs32: as pd_step_sac.  No host synchronisation; the position lives on the device, so
 *  a captured graph replays correctly. */
pd_status pd_step_sac_ring(pd_env* env, const float* heads, int32_t deterministic, float log_std_min,
                           float log_std_max, float max_action, float* eps_out, float* action, float* ring,
                           int64_t capacity, long long* ring_state, float* priorities, const float* max_priority,
                           float* obs32, void* stream);
/* The SAC Actor's forward pass (sac_pytorch.py:129-159) for n float32 observations [n][state_dim]
 * in one launch: Linear(S, H) ReLU, (n_hidden_layers - 1) x [Linear(H, H) ReLU] on MFMA
 * (v_mfma_f32_16x16x4_f32), then the mean and log_std heads into heads [n][2A] (mean | log_std,
 * unclamped: pd_step_sac_ring clamps).  params: a host array of 2 (n_hidden_layers + 2) device
 * pointers, the torch parameters in named_parameters() order (weight [out][in] row-major, bias):
 * shared_net layers, then mean, then log_std.  hidden 128, 256 or 512 (else PD_ERR_UNSUPPORTED),
 * state_dim <= 16, action_dim <= 8, n_hidden_layers <= 8; every parameter 16-byte aligned (else
 * PD_ERR_UNSUPPORTED).  f32 sums in another order than torch's GEMMs: equal to f32 rounding.  Runs
 * on the current HIP device.  n = 0: PD_OK without a launch (obs and heads may be NULL then). */
pd_status pd_sac_actor(int64_t n, int32_t state_dim, int32_t hidden, int32_t n_hidden_layers, int32_t action_dim,
                       const float* obs, const float* const* params, float* heads, void* stream);
/* The whole SAC collection step (sac_pytorch_powered_descent.py:160-183: actor.sample on the
 * current observation, env.step, buffer.add) in ONE launch: pd_sac_actor's forward pass
 * (sac_pytorch.py:129-159) runs in the step kernel's prologue for each workgroup's 16 envs, on
 * obs32 [N][S] as the previous step (or pd_observe) left it, then pd_step_sac_ring follows with
 * those heads (same arguments and semantics; obs32 is overwritten with the next observation).
 * state_dim / action_dim / hidden / n_hidden_layers / params as pd_sac_actor (state_dim and
 * action_dim must equal the handle's pd_obs_dim / pd_action_dim: PD_ERR_INVALID otherwise); heads
 * [N][2A] (may be NULL) receives the heads.  Handles stepping 16 lanes per env (the default up to
 * 4 096 envs) with hidden <= 256 take the single launch; others run pd_sac_actor +
 * pd_step_sac_ring (two launches, the same bits).  No host synchronisation. */
pd_status pd_step_sac_fused(pd_env* env, int32_t state_dim, int32_t action_dim, int32_t hidden,
                            int32_t n_hidden_layers, const float* const* params,
                            float* heads, int32_t deterministic, float log_std_min, float log_std_max,
                            float max_action, float* eps_out, float* action, float* ring, int64_t capacity,
                            long long* ring_state, float* priorities, const float* max_priority, float* obs32,
                            void* stream);
/* Evaluation rollouts of a SAC actor, whole episodes on the device: the driver's evaluate_agent
 * (sac_pytorch_powered_descent.py:234-251: reset, select_action(state, deterministic=True) until
 * done or truncated, total_reward += reward, done counted as a landing) and the loop of
 * visualize_trajectory (:354-376, which keeps the traces), one env per episode.  The actor's
 * forward pass (pd_sac_actor's, the same bits) runs INSIDE the fused-step loop of the step kernel,
 * once per step, on the float32 observation of the env's register state; sampling and the step
 * are pd_step_sac_fused's: the results equal a loop of pd_step_sac_fused calls bit for bit.
 *  state_dim .. params: as pd_step_sac_fused (same checks); hidden 128 or 256
 *  deterministic: != 0: action = tanh(mean) max_action; 0: eps drawn in the kernel as
 *            pd_step_sac_ring draws it (Philox keyed by env, episode, step)
 *  reset_first: != 0: every env is reset first, as by pd_reset; 0: the episodes start from the
 *            handle's current state (pd_set_state, a checkpoint, a previous capped call)
 *  max_steps: the cap on every episode's length in this call
 *  ret     : [N] handle precision, the rewards added in step order; steps: [N] int32 episode
 *            lengths; done: [N] uint8, the terminal step's done; trunc_id: [N] int8, the terminal
 *            step's truncation id.  ret and steps are zeroed at the call's start.
 *  actions_out: [max_steps][N][A] float32; rewards_out: [max_steps][N] handle precision; row t
 *            of env i is written only for t < steps[i]
 *  Each of the six outputs may be NULL.
 * An env whose step returns done or truncated is stored once with its terminal (pre-reset) state
 * and freezes: it is never auto-reset, whatever pd_config.auto_reset says.  An env that reaches
 * max_steps without ending has steps = max_steps, done = 0, trunc_id as its last step left it and
 * the state after max_steps steps; a following call with reset_first = 0 continues it
 * bit-identically.  The rollout is a chain of launches of at most pd_tuning.step_fuse steps (each
 * inserting the neighbourhoods it solved); a workgroup leaves a launch's step loop once none of
 * its 16 envs is live.  Results do not depend on step_fuse.  No host synchronisation.
 * Handle requirements: those of pd_step_sac_fused (RL landing burns, reference integrator,
 * float32 actions).  PD_ERR_UNSUPPORTED, with nothing launched and the cause in pd_last_error, for
 * a handle that does not step 16 lanes per env and for hidden 512 (callers take the per-step
 * path: pd_step_sac_fused / pd_step_sac_ring).  (additive export, ABI 11) */
pd_status pd_rollout_sac(pd_env* env, int32_t state_dim, int32_t action_dim, int32_t hidden,
                         int32_t n_hidden_layers, const float* const* params, int32_t deterministic,
                         float log_std_min, float log_std_max, float max_action, int32_t reset_first,
                         int32_t max_steps, void* ret, int32_t* steps, uint8_t* done, int8_t* trunc_id,
                         float* actions_out, void* rewards_out, void* stream);
/* SAC data collection, n_steps steps of every env per call: the driver's collection loop
 * (sac_pytorch_powered_descent.py:160-183: select_action, env.step, buffer.add, reset at an
 * episode's end) for the span between two learner updates, during which the actor is fixed.  The
 * call is n_steps consecutive pd_step_sac_fused steps -- the actor's forward pass (sac_pytorch.py:
 * 129-159), Actor.sample (:161-179), the env step, the replay row (:27-35) with its priority
 * (:76-83) -- with the actor INSIDE the step kernel's fused-step loop, as in pd_rollout_sac: a chain
 * of launches of at most pd_tuning.step_fuse steps, no host synchronisation, no allocation.  The
 * results equal a loop of n_steps pd_step_sac_fused calls bit for bit, and do not depend on
 * step_fuse or on how the steps are split into calls.
 *  state_dim .. params, deterministic, log_std_min / log_std_max, max_action: as pd_rollout_sac
 *            (same checks; hidden 128 or 256); eps is drawn as pd_step_sac_ring draws it (Philox
 *            keyed by env, episode, step)
 *  Envs auto-reset per pd_config.auto_reset, as in pd_step_sac_fused; none freezes.
 *  ring, ring_state != NULL (ring mode): the replay buffer's rows [capacity][2S + A + 2]; step t's
 *            row of env i goes to (ring_state[0] + t N + i) mod capacity with priorities[row] =
 *            *max_priority (priorities may be NULL); each launch's last workgroup advances
 *            ring_state[0] (position) and ring_state[1] (size, capped at capacity) by its steps x N;
 *            ring_state[2] must be 0 between launches.  n_steps x N <= capacity (the workgroups of
 *            one launch run at different steps: its rows must not alias) and capacity x (2S + A + 2)
 *            < 2^32, else PD_ERR_INVALID
 *  ring, ring_state == NULL (slab mode, for ranks that gather): ring is [n_steps][N][2S + A + 2];
 *            capacity and priorities are ignored; n_steps x N x (2S + A + 2) < 2^32
 *  obs32   : [N][S] float32, OUTPUT ONLY (may be NULL): the observation the actor sees next, after
 *            any reset, after the last step.  Unlike pd_step_sac_fused, which reads obs32 as the
 *            previous step left it, the first step's observation is formed from the handle's
 *            register state -- the value a preceding step or pd_observe, cast to float32, would have
 *            left there
 *  eps_out : [n_steps][N][A] float32; reward: [n_steps][N] handle precision; done, truncated:
 *            [n_steps][N] uint8; trunc_id: [n_steps][N] int8 -- pd_step_n's per-step outputs (the
 *            episode ends the in-kernel resets would otherwise hide).  Each may be NULL.
 *  n_steps == 0: PD_OK, nothing launched or written (the actor and the handle are still checked,
 *            ring and the outputs are not looked at and may be NULL); n_steps < 0: PD_ERR_INVALID.
 * Handle requirements: those of pd_rollout_sac.  PD_ERR_UNSUPPORTED, with nothing launched and the
 * cause in pd_last_error, for a handle that does not step 16 lanes per env and for hidden 512
 * (callers loop pd_step_sac_fused).  (additive export, ABI 11) */
pd_status pd_collect_sac(pd_env* env, int32_t state_dim, int32_t action_dim, int32_t hidden,
                         int32_t n_hidden_layers, const float* const* params, int32_t deterministic,
                         float log_std_min, float log_std_max, float max_action, int32_t n_steps,
                         float* ring, int64_t capacity, long long* ring_state, float* priorities,
                         const float* max_priority, float* obs32, float* eps_out, void* reward,
                         uint8_t* done, uint8_t* truncated, int8_t* trunc_id, void* stream);
/* Multi-step rollout with device-resident actions [T][N][A]: the fused launches of pd_step_n
 * (per-step launches for the other phases), rewards accumulated into reward_sum [N] (may be
 * NULL), no per-step outputs.  No host synchronisation. */
pd_status pd_rollout(pd_env* env, const void* actions, int32_t n_steps, void* reward_sum,
                     void* stream);
/* PSO objective for a batch of particles, one env per particle, on the device:
 * pso_wrapped_env.objective_function (env_wrapped_ea.py:200-222) driven by simple_actor
 * (env_wrapped_ea.py:18-44) evaluated inside the step kernel.  Resets every env, then steps
 * each until done or truncated (or max_steps), accumulating fitness = -sum(reward).
 *  weights : [n_params][N] float32, parameter-major (named_parameters() order per particle);
 *            the rollout first copies them into chunks of four parameters ([ceil(P/4)][N][4],
 *            handle-owned) that the step kernel's actor reads with 16-byte loads
 *  n_params: PD_ACTOR_PARAMS_* for the handle's phase; the handle must have rtd = PD_RTD_PSO
 *  fitness : [N] (handle precision); steps: [N] int32 episode lengths (may be NULL)
 *  check_every: >0 = read the live-env count every that many steps (at least once per launch),
 *            stop early when all envs are done, and size later launches to the live count (one
 *            host sync per check); 0 = always max_steps steps over the full grid.
 * Each launch runs up to 64 fused steps (pd_tuning.policy_fuse); a finished episode's lanes freeze
 * and a wave whose episodes have all ended leaves the launch.  Grids beyond one chip round of lanes
 * step only the live envs (pd_tuning.policy_list): a compacted index list, rebuilt inside the step
 * kernel (wave ballot + prefix count, one atomic per wave).  Results do not depend on either.
 * A refill rollout (pd_tuning.policy_refill; the default for windless swarms) is ONE launch that
 * steps the whole swarm: it reads no live count, so check_every, policy_list and policy_list_at
 * apply only when refill is off (an explicit policy_list >= 0 or policy_list_at > 0 with
 * policy_refill -1 turns it off). */
pd_status pd_rollout_policy(pd_env* env, const float* weights, int32_t n_params, int32_t max_steps,
                            void* fitness, int32_t* steps, int32_t check_every, void* stream);
/* pd_rollout_policy with the weights already in the chunked layout, weights4 [ceil(n_params/4)][N][4]
 * float32 (chunk c of particle i holds parameters 4c .. 4c+3, zeros past n_params; 16-byte aligned):
 * the layout pd_pso_step_chunked writes, so the rollout skips its copy pass.  Same results. (ABI 11) */
pd_status pd_rollout_policy_chunked(pd_env* env, const float* weights4, int32_t n_params, int32_t max_steps,
                                    void* fitness, int32_t* steps, int32_t check_every, void* stream);
/* One PSO generation's particle update on the device (particle_swarm_optimisation.py:437-441
 * personal best, :515-519 update_velocity_with_local_best, :112-118 update_position), binary64:
 *   if fitness < best_fitness: best_position = position;  best_fitness = min(best_fitness, fitness)
 *   v = w v + c1 r1 (best_position - x) + c2 r2 (swarm_best[swarm] - x);  x = clip(x + v, lower, upper)
 * r1, r2: one uniform per particle and generation (Philox4x32-10 keyed by seed, counter
 * (particle_offset + p, generation)).  Arrays are parameter-major [dim][n_particles]; swarm_best
 * [n_swarms][dim]; swarm [n_particles] int32 subswarm ids; lower/upper [dim].  position_f32
 * (optional, [dim][n_particles]) receives the new positions as the float32 actor weights
 * pd_rollout_policy reads.  Device pointers; runs on the current HIP device. */
pd_status pd_pso_step(int64_t n_particles, int32_t dim, const double* fitness, double* best_fitness,
                      double* position, double* velocity, double* best_position, const double* swarm_best,
                      const int32_t* swarm, const double* lower, const double* upper, double w, double c1,
                      double c2, uint64_t seed, uint32_t generation, uint64_t particle_offset,
                      float* position_f32, void* stream);
/* pd_pso_step with the float32 copy in the chunked layout of pd_rollout_policy_chunked:
 * position_f32_chunked (required) [ceil(dim/4)][n_particles][4], zeros past dim.  One thread per
 * (chunk, particle) updates its four parameters with the same operations as pd_pso_step (the same
 * bits in position, velocity, best_position and best_fitness) and stores the chunk with one 16-byte
 * store. (ABI 11) */
pd_status pd_pso_step_chunked(int64_t n_particles, int32_t dim, const double* fitness, double* best_fitness,
                              double* position, double* velocity, double* best_position, const double* swarm_best,
                              const int32_t* swarm, const double* lower, const double* upper, double w, double c1,
                              double c2, uint64_t seed, uint32_t generation, uint64_t particle_offset,
                              float* position_f32_chunked, void* stream);
/* Per subswarm s < n_swarms, the first particle of minimal fitness among those with swarm[p] ==
 * s: the result of particle_swarm_optimisation.py:437-441's sequential `if fitness <
 * subswarm_best` over the subswarm's particles in order (a NaN fitness never wins, ties keep the
 * lower index): min_fitness [n_swarms] and its position min_position [n_swarms][dim] (from
 * position [dim][n_particles]); +inf and zeros for a subswarm with no particle of non-NaN fitness.
 * A two-pass segmented argmin over blocks of 1 024 particles; no host synchronisation.  scratch:
 * a device buffer of at least pd_pso_swarm_minima_scratch_bytes(n_particles, n_swarms) bytes for
 * the first pass's partials, owned by the caller (calls that may overlap need their own). */
size_t pd_pso_swarm_minima_scratch_bytes(int64_t n_particles, int32_t n_swarms);
pd_status pd_pso_swarm_minima(int64_t n_particles, int32_t dim, int32_t n_swarms, const double* fitness,
                              const int32_t* swarm, const double* position, double* min_fitness,
                              double* min_position, void* scratch, size_t scratch_bytes, void* stream);
/* The subswarm and global bests after a generation (particle_swarm_optimisation.py:442-444,
 * :474-477), on the device: subswarm s takes (min_fitness[s], min_position[s]) if strictly better;
 * then the first subswarm holding the smallest best replaces global_best(_fitness) if strictly
 * better.  swarm_best [n_swarms][dim], global_best [dim], the fitnesses [n_swarms] / [1]. */
pd_status pd_pso_update_bests(int32_t n_swarms, int32_t dim, const double* min_fitness, const double* min_position,
                              double* swarm_best_fitness, double* swarm_best, double* global_best_fitness,
                              double* global_best, void* stream);
/* Prioritized replay on the device: the learner's sample and priority update of the reference's
 * PrioritizedReplayBuffer (sac_pytorch.py:90-124) without the host.  No env handle: device pointers,
 * the current HIP device, no host synchronisation, nothing read back.  (additive exports, ABI 11)
 *
 * pd_per_sample draws `batch` distinct items of priorities[0, size) with probability proportional
 * to priority^alpha, without replacement: the distribution of np.random.choice(size, batch,
 * replace=False, p=prio**alpha / sum) (sac_pytorch.py:96-101), as an exponential race.
 *  weight  : w_i = pow((double)priorities[i], alpha); an item takes part only if 0 < w_i < inf
 *            (a zero, negative or NaN priority is never drawn)
 *  uniform : one Philox4x32-10 block per pair of items, m = i >> 1: counter {lo32(m), lo32(draw),
 *            hi32(draw), 48}, key (lo32(seed), hi32(seed)); u_i = 1 - u01(x, y) for even i and
 *            1 - u01(z, w) for odd i, in (0, 1].  A sample depends on (seed, draw, priorities) only
 *  key     : e_i = -log(u_i) / w_i in binary64, +inf for an item that takes no part
 *  indices : [batch] the items with the smallest keys, ties to the lower index, slot j the j-th
 *            smallest -- the order of numpy's sequential draw
 *  weights : [batch] float32 (size w_j / sum w)^-beta / (the largest of the batch)
 *            (sac_pytorch.py:104-108), computed as (w_ref / w_j)^beta in binary64 with w_ref the
 *            smallest selected weight (the sum over the buffer cancels); the largest is exactly 1
 *  rows    : [batch][width] = ring[indices[j]] bit for bit (sac_pytorch.py:110-116); ring and rows
 *            may be NULL
 *  keys_out: optional [size], receives every e_i
 *  info    : [4] int32: slots filled = min(batch, finite keys); finite keys; 1 if the internal
 *            candidate list overflowed (candidates were dropped: never in a correct run); 0.
 *            Slots past info[0] get index -1, weight 0 and zero rows
 *  scratch : at least the bytes the scratch-size call below returns for (size, batch), 8-byte
 *            aligned, owned by the caller; the call initialises what it reads of it
 * PD_ERR_INVALID for a NULL priorities / indices / weights / info / scratch, size < 1, batch < 1,
 * batch > size, rows without ring, a ring with width < 1, alpha < 0, a non-finite alpha or beta, a
 * short or misaligned scratch; PD_ERR_UNSUPPORTED for batch > PD_PER_MAX_BATCH or size >= 2^31;
 * all before any launch.
 *
 * pd_per_update (sac_pytorch.py:120-124): priorities[indices[j]] = fabsf(td_errors[j]) + epsilon
 * (a float32 add) for every j with 0 <= indices[j] < size -- other indices, the -1 of a short sample
 * among them, are skipped -- and *max_priority raised to the largest written value that compares
 * greater (an integer atomic max on the bit pattern: priorities are non-negative; a NaN never raises
 * it).  Indices are distinct by contract; of duplicates, one written value survives. */
#define PD_PER_MAX_BATCH 1024
size_t pd_per_sample_scratch_bytes(int64_t size, int32_t batch);
pd_status pd_per_sample(const float* priorities, int64_t size, int32_t batch, double alpha, double beta,
                        uint64_t seed, uint64_t draw, const float* ring, int32_t width, int64_t* indices,
                        float* weights, float* rows, double* keys_out, int32_t* info, void* scratch,
                        size_t scratch_bytes, void* stream);
pd_status pd_per_update(float* priorities, int64_t size, const int64_t* indices, const float* td_errors,
                        int32_t batch, float epsilon, float* max_priority, void* stream);
/* The inference-only third of the SAC update on the device (additive exports, ABI 11).  No env
 * handle: device pointers, the current HIP device, no host synchronisation, nothing read back.
 *
 * pd_sac_critic: Critic.forward (sac_pytorch.py:181-221) for n rows in one launch: q [n][2], Q1 in
 * column 0 and Q2 in column 1, of cat([state, action]); each net Linear(S + A, H) ReLU,
 * (n_hidden_layers - 1) x [Linear(H, H) ReLU], Linear(H, 1), float32 throughout, on pd_sac_actor's
 * code (MFMA hidden layers, activations in LDS), the two nets in workgroups of their own.
 * states [n][S], actions [n][A]; params_q1 / params_q2: host arrays of 2 (n_hidden_layers + 1)
 * device pointers each, the torch parameters of q1 / q2 in named_parameters() order.
 * state_dim >= 1, action_dim >= 1, state_dim + action_dim <= 16, n_hidden_layers 1..8, n >= 0, no
 * null pointer (else PD_ERR_INVALID); hidden 128, 256 or 512 and every parameter 16-byte aligned
 * (else PD_ERR_UNSUPPORTED); all before any launch.  n = 0: PD_OK without a launch (states,
 * actions and q may be NULL then). */
pd_status pd_sac_critic(int64_t n, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t n_hidden_layers,
                        const float* states, const float* actions, const float* const* params_q1,
                        const float* const* params_q2, float* q, void* stream);
/* pd_sac_td_target: the torch.no_grad() block of SACPyTorch.update (sac_pytorch.py:439-443) for a
 * sampled batch in ONE launch:
 *     next_actions, next_log_probs = actor.sample(next_states)
 *     next_q1, next_q2 = critic_target(next_states, next_actions)
 *     next_q = min(next_q1, next_q2) - alpha * next_log_probs
 *     target_q = rewards + (1 - dones) * gamma * next_q
 *  rows    : [batch][width], the replay buffers' row layout state | action | reward | next_state |
 *            done, width = 2 state_dim + action_dim + 2 (any other width: PD_ERR_INVALID), as
 *            pd_per_sample leaves them; read once
 *  actor   : actor_hidden, actor_layers, actor_params as pd_sac_actor's hidden, n_hidden_layers and
 *            params; log_std_min, log_std_max, max_action as pd_step_sac_ring's
 *  critic  : critic_hidden, critic_layers, params_q1, params_q2 as pd_sac_critic's (the TARGET critic)
 *  log_alpha: a device scalar; alpha = expf(*log_alpha), read by the kernel
 *  eps     : eps_in [batch][A], or NULL: drawn in the kernel, Philox4x32-10 with key (lo32(seed),
 *            hi32(seed)) and counter {lo32(row), lo32(draw), hi32(draw), 64 + k / 2}, components 2m
 *            and 2m + 1 of a row from one block by Box-Muller in binary64 (u1 = 1 - u01(x, y),
 *            u2 = u01(z, w), sqrt(-2 log u1) (cos, sin)(2 pi u2)), cast to float32: a draw depends on
 *            (seed, draw, row, k) only
 * In float32, in torch's operation order:
 *  heads   = Actor.forward(next_state), unclamped: pd_sac_actor's bits on the same rows
 *  ls = clamp(log_std, min, max), sd = expf(ls), x = mean + sd eps, a = tanhf(x),
 *  next_actions = a max_action (Actor.sample, sac_pytorch.py:166-179)
 *  next_log_prob = sum over k ascending of -((x - mean)^2) / (2 sd^2) - ls - log(sqrt(2 pi))
 *            - logf(1 - a^2 + 1e-6f)   (Normal.log_prob and the tanh correction, :173-177)
 *  next_q  = [batch][2]: pd_sac_critic's bits on (next_state, next_actions)
 *  target_q = reward + ((1 - done) gamma) (fminf(q1, q2) - alpha next_log_prob)   [batch]; no
 *            special case for done = 1 with a non-finite next_q (torch has none)
 * target_q is required; next_actions [batch][A], next_log_prob [batch], next_q [batch][2], heads
 * [batch][2A] and eps_out [batch][A] may each be NULL.  Any batch >= 0 (0: PD_OK without a launch).
 * PD_ERR_INVALID for a negative batch, a dimension below 1, a wrong width or a null rows / target_q
 * (batch > 0) / log_alpha / parameter; PD_ERR_UNSUPPORTED for shapes outside the two nets' domains
 * (state_dim + action_dim > 16, action_dim > 8, layers outside 1..8, a hidden width other than 128,
 * 256, 512, a parameter not 16-byte aligned); all before any launch. */
pd_status pd_sac_td_target(int64_t batch, int32_t state_dim, int32_t action_dim, const float* rows, int32_t width,
                           int32_t actor_hidden, int32_t actor_layers, const float* const* actor_params,
                           float log_std_min, float log_std_max, float max_action, int32_t critic_hidden,
                           int32_t critic_layers, const float* const* params_q1, const float* const* params_q2,
                           const float* log_alpha, float gamma, uint64_t seed, uint64_t draw, const float* eps_in,
                           float* target_q, float* next_actions, float* next_log_prob, float* next_q, float* heads,
                           float* eps_out, void* stream);
/* The critic step of SACPyTorch.update on the device (csrc/pdsacupd.hip), in three launches and
 * without a host synchronisation: pd_sac_critic_grad (two launches) replaces sac_pytorch.py:445-471
 * -- critic(states, actions), the four losses of :457-468, critic_optimizer.zero_grad() and
 * critic_loss.backward() -- and the |td| of :526; pd_adam_step (one launch) replaces :474-483 and
 * :530-531 -- clip_grad_norm_, critic_optimizer.step() and the Polyak loop.  All float32; no float
 * atomics: every sum has a fixed order, so the same inputs give the same bits on every call.
 *
 * Scratch of pd_sac_critic_grad: with Bp = 16 ceil(batch / 16), the post-ReLU activations and the
 * deltas of every layer of both nets [2][L][Bp][H] each, the two nets' dq and |target - q| [2][Bp]
 * each and the row tiles' loss partials [Bp / 16][2]:
 *   bytes = 4 (4 L H Bp + 4 Bp + Bp / 8)
 * (0 for a batch, hidden or n_hidden_layers below 1).  Owned by the caller, 16-byte aligned; calls
 * that may overlap need their own. */
#define PD_SAC_LOSS_L2 0   /* F.mse_loss: per-row dq = 2 w (q - target) / B */
#define PD_SAC_LOSS_L1 1   /* F.l1_loss:  per-row dq = w sign(q - target) / B, sign(0) = 0 */
#define PD_ADAM_MAX_TENSORS 64
size_t pd_sac_critic_grad_scratch_bytes(int64_t batch, int32_t hidden, int32_t n_hidden_layers);
/* q = critic(state | action), the loss and its gradient with respect to every parameter of both
 * Q nets.  sa: state | action are the first state_dim + action_dim floats of each of `batch` rows
 * `pitch` floats apart (pitch = the row width W for a buffer's last_rows, state_dim + action_dim for
 * a packed tensor).  target_q [batch]; weights [batch], the PER importance weights, or NULL (w = 1);
 * loss_kind PD_SAC_LOSS_L2 / _L1: with the weights or without, the four losses of
 * sac_pytorch.py:457-468.  dq_in [batch][2] or NULL: given, it is the upstream gradient dLoss/dq of
 * (row, net) in place of the loss's own (target_q may then be NULL when neither td_abs nor loss_out
 * is asked for).  params_q1 / params_q2 as pd_sac_critic's; grads_q1 / grads_q2: the gradient
 * tensors (p.grad) in the same order, OVERWRITTEN, never accumulated into (zero_grad() + backward()).
 * Outputs, each may be NULL: q [batch][2] (pd_sac_critic's bits), td_abs [batch] = max(|target - q1|,
 * |target - q2|), dq_out [batch][2], loss_out [1] (the mean over the batch: (w l1 + w l2).mean() with
 * weights, mean(l1) + mean(l2) without; the loss_kind's loss also under dq_in), sumsq_partials: one
 * sum of squares of gradient elements per workgroup of the second launch, 2 (H / 64 + (L - 1) (H / 16)
 * (H / 128) + H / 128) of them -- *n_partials holds the array's length on entry (PD_ERR_INVALID if
 * too short) and that count on return (0 for an empty batch); their sum in index order is the
 * squared norm pd_adam_step clips by.
 * Domain: pd_sac_critic's (state_dim + action_dim <= 16, hidden 128 / 256 / 512, 1 to 8 hidden
 * layers, parameters and gradients 16-byte aligned).  PD_ERR_INVALID: a negative batch, a dimension
 * out of range, pitch below state_dim + action_dim, an unknown loss kind, a null required pointer,
 * scratch missing, misaligned or short; PD_ERR_UNSUPPORTED: another hidden width, a misaligned
 * parameter or gradient; all before any launch.  batch == 0: PD_OK, nothing launched. */
pd_status pd_sac_critic_grad(int64_t batch, int32_t state_dim, int32_t action_dim, int32_t hidden,
                             int32_t n_hidden_layers, const float* sa, int32_t pitch, const float* target_q,
                             const float* weights, int32_t loss_kind, const float* dq_in,
                             const float* const* params_q1, const float* const* params_q2, float* const* grads_q1,
                             float* const* grads_q2, float* q, float* td_abs, float* dq_out, float* loss_out,
                             float* sumsq_partials, int32_t* n_partials, void* scratch, size_t scratch_bytes,
                             void* stream);
/* clip_grad_norm_ (sac_pytorch.py:474-479), torch.optim.Adam.step (:483; no weight decay, no
 * amsgrad) and the Polyak loop (:530-531) over a list of n_tensors <= PD_ADAM_MAX_TENSORS float32
 * tensors in one launch (the host arrays are read during the call; numel[k] elements each, any
 * alignment, a tensor of 0 elements is skipped).
 *   max_norm > 0: total = sqrt(sum of sumsq_partials[0 .. n_partials) in index order), coef = min(1,
 *                 max_norm / (total + 1e-6)), grads *= coef in place, grad_norm_out[0] = total (may
 *                 be NULL); max_norm <= 0: no clipping, the gradients and grad_norm_out untouched;
 *   Adam:         m = m + fl(1 - beta1) (g - m); v = beta2 v + (fl(1 - beta2) g) g;
 *                 p = p - step_size (m / (sqrt(v) / bc2_sqrt + eps)), with step_size = lr / (1 -
 *                 beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) computed by the caller in binary64 from
 *                 the step count t (after its increment) and rounded to float32 here;
 *   targets:      NULL, or n_tensors target tensors: t = fl(1 - tau) t + fl(tau) p on the new p, two
 *                 rounded products and their rounded sum (torch's (1 - tau) * t + tau * p).
 * PD_ERR_INVALID: n_tensors out of range, a null list or tensor, a negative numel, clipping
 * without partials; before any launch. */
pd_status pd_adam_step(int32_t n_tensors, float* const* params, float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, const int64_t* numel, float* const* targets, double step_size,
                       double bc2_sqrt, double beta1, double beta2, double eps, double max_norm,
                       const float* sumsq_partials, int32_t n_partials, float* grad_norm_out, double tau, void* stream);
/* The gradient of each Q net of the twin critic with respect to its input, with unit upstream
 * gradient (the actor step's way through the critic, sac_pytorch.py:487-497), in one launch over
 * batch rows of state | action (the first state_dim + action_dim floats of a row, rows pitch floats
 * apart, as pd_sac_critic_grad takes them).  Outputs, each may be NULL: q [batch][2] (pd_sac_critic's
 * bits) and dsa [batch][2][state_dim + action_dim], dsa[b][k][c] = d q_k / d input_c.
 * Order of operations (float32): the forward pass is pd_sac_critic's; delta_{L-1}[j] = wm[j] (h_{L-1}[j]
 * > 0); delta_{l-1} = (delta_l . W_l) (h_{l-1} > 0) as pd_sac_critic_grad's chain (k ascending over W_l's
 * rows, one rounding per fma step); dsa[c] = sum_j delta_0[j] W1[j][c] in 16 parts of H / 16 consecutive
 * j, fma in ascending j within a part from 0, the parts joined by the head stage's tree (p ^ 8, ^ 4, ^ 2,
 * ^ 1).  On integer nets every step is exact.  No deltas are stored and no scratch is needed: the layers'
 * signs are kept in LDS.  Domain and refusals: pd_sac_critic's, and PD_ERR_INVALID for a pitch below
 * state_dim + action_dim; all before any launch.  batch == 0: PD_OK, nothing launched. */
pd_status pd_sac_critic_dinput(int64_t batch, int32_t state_dim, int32_t action_dim, int32_t hidden,
                               int32_t n_hidden_layers, const float* sa, int32_t pitch, const float* const* params_q1,
                               const float* const* params_q2, float* q, float* dsa, void* stream);
/* Bytes of scratch pd_sac_actor_grad needs: 4 (Bp (2 L H + 5 A + 19) + Bp / 8) with Bp = 16 ceil(batch /
 * 16), H = actor_hidden, L = actor_layers, A = action_dim (the actor's post-ReLU tiles and deltas, and
 * per row the head gradients padded to 16, heads, eps, dq/da, q, log_prob; two loss partials a row tile;
 * the critic needs none).  0 for a non-positive argument. */
size_t pd_sac_actor_grad_scratch_bytes(int64_t batch, int32_t action_dim, int32_t actor_hidden, int32_t actor_layers);
/* The actor and temperature steps of SACPyTorch.update up to the optimizers (sac_pytorch.py:485-497 and
 * :512-520): actor.sample(states), critic(states, new_actions) with the CURRENT critic, min(q1, q2), the
 * actor loss with PER weights (weights [batch]) or without (NULL), zero_grad() + backward() through both
 * Q nets into the actor, and the temperature loss and its gradient; three launches, no host
 * synchronisation, no atomics.  The optimizer steps are pd_adam_step's: one call over the actor's
 * tensors with sumsq_partials for the clip, one over the one-element log_alpha with log_alpha_grad.
 * rows: batch rows, pitch floats apart, whose first state_dim floats are the state (a replay sample's
 * [B][2S + A + 2] rows, or packed states).  actor_params / actor_grads: pd_sac_actor's order (w, b of
 * each hidden layer, mean.weight, mean.bias, log_std.weight, log_std.bias); the gradients are
 * overwritten, never accumulated.  log_alpha: a device float32 scalar, read once (alpha =
 * expf(*log_alpha)); no launch of this call writes it.  eps_in [batch][A] or NULL: drawn, Philox4x32-10
 * with key (lo32(seed), hi32(seed)) and counter (row, lo32(draw), hi32(draw), 72 + k / 2), Box-Muller as
 * pd_sac_td_target -- the tag differs (64 there), so the same (seed, draw) gives noise independent of the
 * TD target's.  dheads_in [batch][2A] or NULL: given, it replaces dLoss / d(mean | raw log_std); the
 * critic pointers may then be NULL and q, dq_da and actor_loss are not written.
 * Per row b and component k, float32 in this order (w = weights[b] or 1, Bf = (float)batch):
 *   heads            Actor.forward(state), unclamped: pd_sac_actor's bits
 *   sample           raw = log_std head; ls = clamp(raw, lo, hi); sd = expf(ls); x = m + sd eps; a =
 *                    tanhf(x); new_action = a max_action; log_prob = sum_k (-(d d) / (2 (sd sd)) - ls -
 *                    0.9189385332046727 - logf(1 - a a + 1e-6)), d = x - m, k ascending: pd_sac_td_target's
 *                    bits for the same state and eps
 *   q_j              Q_j(state | new_action), j = 1, 2: pd_sac_critic's bits
 *   dq_da[j][k]      pd_sac_critic_dinput's action columns
 *   coefficients     sel_j = 1 for the smaller q, 0 for the larger, 1/2 each on a tie (torch.min's
 *                    backward); c_j = -((w / Bf) sel_j); cl = (w alpha) / Bf
 *   sample backward  t = 1 - a a; G = c_1 dq_da[1][k] + c_2 dq_da[2][k]; gx = (G max_action) t + cl (((2 a) t)
 *                    / (t + 1e-6)); dmean = gx; draw = ((gx sd) eps - cl) if lo <= raw <= hi (torch.clamp
 *                    passes the gradient at both bounds), else 0.  The two paths of Normal.log_prob's
 *                    quadratic term, through x and through mean / std, cancel analytically ((x - m) / sd is
 *                    eps) and are left out; float32 autograd keeps their rounding residue.
 *   actor backward   delta_{L-1}[j] = (fma chain from 0 over dmean_k Wm[k][j], k ascending, then draw_k
 *                    Ws[k][j], k ascending) (h_{L-1}[j] > 0); the hidden chain as pd_sac_critic_grad's; dW_l
 *                    = delta_l^T h_{l-1} with the batch rows added in ascending order, four an MFMA
 *                    instruction; [dWm ; dWs] one row tile of 2A rows; the biases the column sums.
 *   losses           per row la = w (alpha log_prob - fminf(q1, q2)), lt = w (log_prob + target_entropy);
 *                    the 16 rows of a tile added in ascending order, the tiles in ascending order;
 *                    actor_loss = S_la / Bf; log_alpha_grad = -(S_lt / Bf); alpha_loss = log_alpha
 *                    log_alpha_grad (sac_pytorch.py:515-517).
 * Outputs, each may be NULL: new_actions [B][A], log_prob [B], q [B][2], heads [B][2A], eps_out [B][A],
 * dq_da [B][2][A], dheads_out [B][2A] (dmean | draw), actor_loss [1], alpha_loss [1], log_alpha_grad [1],
 * sumsq_partials: one sum of squares per workgroup of the third launch, H / 64 + (L - 1) (H / 16) (H /
 * 128) + H / 128 of them for the actor's H and L, under pd_sac_critic_grad's protocol for *n_partials.
 * Domain: pd_sac_actor's (state_dim <= 16, action_dim <= 8, hidden 128 / 256 / 512, 1 to 8 hidden
 * layers) and, unless dheads_in is given, pd_sac_critic's with input state_dim + action_dim <= 16;
 * parameters and gradients 16-byte aligned.  PD_ERR_INVALID: a negative batch, a dimension below 1, pitch
 * below state_dim, a null required pointer, sumsq_partials without n_partials or too short, scratch
 * missing, misaligned or short; PD_ERR_UNSUPPORTED: a dimension or layer count above the domain, another
 * hidden width, a misaligned parameter or gradient; all before any launch.  batch == 0: PD_OK, nothing
 * launched. */
pd_status pd_sac_actor_grad(int64_t batch, int32_t state_dim, int32_t action_dim, const float* rows, int32_t pitch,
                            const float* weights, int32_t actor_hidden, int32_t actor_layers,
                            const float* const* actor_params, float* const* actor_grads, float log_std_min,
                            float log_std_max, float max_action, int32_t critic_hidden, int32_t critic_layers,
                            const float* const* params_q1, const float* const* params_q2, const float* log_alpha,
                            float target_entropy, uint64_t seed, uint64_t draw, const float* eps_in,
                            const float* dheads_in, float* new_actions, float* log_prob, float* q, float* heads,
                            float* eps_out, float* dq_da, float* dheads_out, float* actor_loss, float* alpha_loss,
                            float* log_alpha_grad, float* sumsq_partials, int32_t* n_partials, void* scratch,
                            size_t scratch_bytes, void* stream);
/* pd_sac_learning_stats: steps 9 and 10 of SACPyTorch.update, _track_learning_stats
 * (sac_pytorch.py:553-634), as ONE launch (csrc/pdsacstats.hip; additive exports, ABI 11).  No env
 * handle: device pointers, the current HIP device, no host synchronisation, nothing read back -- the
 * reference makes six device-to-host copies, four .item() calls and about thirty NumPy reductions.
 * out_row [PD_SAC_N_STATS] binary64 receives one row of learning_stats in the reference's key order
 * (sac_pytorch.py:346-397; pd_sac_stat_name(column) returns the key, NULL outside [0, PD_SAC_N_STATS)):
 *   0      step
 *   1-5    state_{mean,min,max,std,kurtosis}    6-10  action_...    11-15  reward_...
 *   16-19  critic_loss, actor_loss, alpha_loss, alpha_value
 *   20-23  q_value_{mean,min,max,std}    24-27  log_prob_...    28-31  target_q_...
 *   32-34  per_beta, per_mean_weight, per_max_priority
 *   35-36  actor_grad_norm, critic_grad_norm
 *  rows    : [batch][width] state | action | reward | ... (a buffer's sampled rows), width >= state_dim
 *            + action_dim + 1; q [batch][2] (the actor step's Q1 | Q2: the statistic is over
 *            fminf(q1, q2)); target_q, log_prob [batch]; weights [batch] or NULL (a uniform buffer)
 *  series  : each state dimension over the batch (state_dim series), all batch x action_dim action
 *            values as one, the reward column, fminf(q1, q2), target_q, log_prob, weights
 *  mean, min, max as np.mean / np.min / np.max; std the population standard deviation (np.std, ddof
 *  0); kurtosis scipy.stats.kurtosis's default (Fisher, biased): m4 / m2^2 - 3 with central moments
 *  divided by n, 0 / 0 = NaN for a constant series.  The five state_* columns are the plain mean over
 *  the state dimensions (ascending) of the per-dimension statistic (:566-583).  A NaN anywhere in a
 *  series makes all that series' statistics NaN, min and max included (NumPy's behaviour).
 *  Arithmetic: every float32 is widened to binary64, all sums are binary64 and two-pass (the mean,
 *  then the central moments about it) in an order fixed by the shape alone; no atomics: the same
 *  inputs give the same bytes on every call.  batch == 1: std 0, kurtosis NaN.
 *  scalars : critic_loss, actor_loss, alpha_loss, max_priority, actor_grad_norm, critic_grad_norm are
 *            device scalars widened exactly; each may be NULL, its column is then NaN.
 *            alpha_value = expf(*log_alpha) (pd_sac_td_target's expf).  per_mean_weight is NaN
 *            without weights, and per_beta too; otherwise per_beta and step are stored as given
 *            (step as a double: exact below 2^53).
 * Only out_row is written.  PD_ERR_INVALID: batch < 1, state_dim < 1, action_dim < 1, width <
 * state_dim + action_dim + 1, a NULL rows / q / target_q / log_prob / log_alpha / out_row;
 * PD_ERR_UNSUPPORTED: state_dim > 16 or action_dim > 8 (the SAC kernels' domain), batch > 65536; all
 * before any launch. */
#define PD_SAC_N_STATS 37
const char* pd_sac_stat_name(int32_t column);
pd_status pd_sac_learning_stats(int64_t batch, int32_t state_dim, int32_t action_dim, const float* rows, int32_t width,
                                const float* q, const float* target_q, const float* log_prob, const float* weights,
                                const float* critic_loss, const float* actor_loss, const float* alpha_loss,
                                const float* log_alpha, const float* max_priority, const float* actor_grad_norm,
                                const float* critic_grad_norm, double per_beta, int64_t step, double* out_row,
                                void* stream);
/* Insert the aero neighbourhoods solved on device and still queued into the handle's tables
 * (one tiny kernel; a no-op when nothing is queued).  Since ABI 10 every step launch (pd_step,
 * pd_step_n, pd_step_sac*, pd_rollout) inserts the neighbourhoods it solved itself, by its last
 * workgroup, and pd_rollout_policy flushes its own: a caller never needs this call any more.
 * It stays for callers written against ABI <= 9 (their periodic flush finds the queue empty). */
pd_status pd_flush_misses(pd_env* env, void* stream);
/* Current observation (post-reset) [N][O]. */
pd_status pd_observe(pd_env* env, void* obs, void* stream);
/* State SoA [11][N] in the handle's precision. */
pd_status pd_get_state(pd_env* env, void* state, void* stream);
pd_status pd_set_state(pd_env* env, const void* state, void* stream);
/* Landing-burn actuator memory [3][N] (gimbal deg, left/right fin command rad). */
pd_status pd_get_actuators(pd_env* env, void* act, void* stream);
pd_status pd_set_actuators(pd_env* env, const void* act, void* stream);
/* g-load history of every env (base_environment.py:137-149: |v| of previous_state and the
 * g_loads_window list, oldest first): vprev [N], window [10][N] (handle precision), len [N]
 * (0..10 valid entries).  Teacher forcing and checkpoint/restore. */
pd_status pd_set_gload_window(pd_env* env, const void* vprev, const void* window, const uint8_t* len,
                              void* stream);
/* g-load history read back: vprev [N], window [10][N] (ring slots), len and head [N] (the oldest
 * entry is slot head when len == 10, slot 0 otherwise). */
pd_status pd_get_gload_window(pd_env* env, void* vprev, void* window, uint8_t* len, uint8_t* head, void* stream);
/* Per-env wind state: sigma_u, sigma_v [2][N] (double). */
pd_status pd_set_wind_sigmas(pd_env* env, const double* sig, void* stream);
/* Wind state (vonkarman.py:33-36 filter states, full_wind_model.py percentile): filters [4][N]
 * (u0 u1 v0 v1, handle precision), sigmas [2][N] (handle precision), profile [N] uint8
 * (percentile - 50).  Any pointer may be NULL.  pd_set_wind_state returns PD_ERR_INVALID, writing
 * nothing, if a profile byte is >= PD_N_WIND_PROFILES (it synchronises the stream to check). */
pd_status pd_get_wind_state(pd_env* env, void* filters, void* sigmas, uint8_t* profile, void* stream);
pd_status pd_set_wind_state(pd_env* env, const void* filters, const void* sigmas, const uint8_t* profile, void* stream);
/* Episode bookkeeping: episode counter and step-within-episode [N] uint32 (the Philox counter
 * words of the wind and reset draws), truncation id [N] int8.  Any pointer may be NULL. */
pd_status pd_get_counters(pd_env* env, uint32_t* episode, uint32_t* step, int8_t* trunc_id, void* stream);
pd_status pd_set_counters(pd_env* env, const uint32_t* episode, const uint32_t* step, const int8_t* trunc_id,
                          void* stream);
/* Checkpoint of every per-env buffer (state, g-load window, actuator memory, wind, counters,
 * aero caches, episode flags) as one opaque device blob of pd_checkpoint_size() bytes: save
 * into, load from a device buffer.  Restoring into a handle of the same configuration continues
 * bit-identically (the Philox draws depend only on (seed, env, episode, step)).  Loading a blob
 * whose wind profile bytes are out of range returns PD_ERR_INVALID and loads nothing. */
size_t pd_checkpoint_size(const pd_env* env);
pd_status pd_checkpoint_save(pd_env* env, void* blob, void* stream);
pd_status pd_checkpoint_load(pd_env* env, const void* blob, void* stream);
/* Counters since create: aero-table misses solved on device, NaN guard hits. Host sync. */
pd_status pd_counters(pd_env* env, int64_t* rbf_misses, int64_t* table_entries_cd,
                      int64_t* table_entries_cl, int64_t* nan_events);
/* The handle's ISA atmosphere (endo_atmospheric_model, atmosphere_dynamics.py:5-27) at n device
 * altitudes [n] (handle precision): out [3][n] = density, pressure, speed of sound.  Used by the
 * facade's maximum_velocity (env_wrapped_rl_pytorch.py:60-66). */
pd_status pd_atmosphere(pd_env* env, const void* altitude, void* out, int64_t n, void* stream);
/* All device statistics words (up to n, at most PD_N_STATS): 0 misses, 1 NaN events, 2/3 table
 * entries C_D/C_L, 16 solved neighbourhoods not queued (queue full; solved again until a later
 * flush).  Workload counters of the step kernel, summed over every launch made with counting on
 * (pd_count_work) since create:
 * 32 env sub-steps inside the gust band (stochastic wind, y < 15 km), 33 in-kernel auto-resets;
 * with 2 lanes per env (one table query per lane and sub-step): 34 queries on a clamped line,
 * 35 queries whose candidate neighbourhood was verified by the swap search, 36 queries evaluated
 * from a Taylor piece, 37 by the balanced chunk sums, 38 missed (device solve), 39 balanced-sum
 * rounds, 40 interior queries in a refined grid cell, 41 ... in a sub-cell split by a bisector,
 * 42 / 43 wave sub-steps with at least one such query, 44 queries evaluated from a cell piece,
 * 45 wave sub-steps holding both clamped-line and interior queries; the carried search intervals,
 * per search a pair of wave sub-step counts -- every lane's carried guess held / the search ran:
 * 46 / 47 wind profile knots, 48 / 49 grid-fin C_a knots.
 * Host sync. */
#define PD_N_STATS 64
pd_status pd_stats(pd_env* env, int64_t* out, int32_t n);
/* Workload counting (pd_stats words 32-49) on (enable != 0) or off (the default) for the handle's
 * following step launches with 2 lanes per env (the default above 16 384 envs; other launches
 * count nothing).  A diagnostic: on, the launches run a counting instantiation of the step kernel
 * (a ballot and an LDS add per counter per sub-step, a few per cent slower); off, the product
 * kernel has no counting code.  Results do not change. */
pd_status pd_count_work(pd_env* env, int32_t enable);
/* Cell pieces of one table (0: C_D, 1: C_L), host only (no device needed): the polynomial + exact-
 * term records that binary64 handles evaluate interior queries from (not a
 * reference interface: the test hook behind them).  Built once per process and table.
 * out[0] pieces, [1] rejected by the build's check, [2] worst checked error relative to
 * sum |c_j phi_j|, [3] build seconds, [4] records, [5] nm, [6] na, [7] a0, [8] a1 (the grid),
 * [9] degree, [10] exact terms, [11] record stride, [12] pieces the binary32 check rejects (of the
 * binary64-valid), [13] its worst error relative to sum |c_j phi_j| + |s|, [14] / [15] exact cells
 * with a valid binary64 / binary32 piece; piece >= 0 (an exact cell's piece is at its
 * cell index im na + ia): its record at out[16 ...] (n_out >= 16 + stride). */
pd_status pd_cell_piece_info(const pd_params* params, int32_t table, int64_t piece, double* out, int32_t n_out);
/* The step kernel's tabulated ISA atmosphere (atmosphere_dynamics.py:5-27), built and evaluated on
 * the host in the device's order and precision (test hook; no device needed): rho, p, a into
 * atm_out [n_alt][3] at geometric altitudes alt; max_rel: the builder's worst relative error
 * against the long double closed form. */
pd_status pd_atm_table(const pd_params* params, int32_t precision, const double* alt, int64_t n_alt,
                       double* atm_out, double* max_rel);
/* The coarse atmosphere table held in LDS by the 512-thread step kernels (binary64 wind handles,
 * pure throttle, two lanes per env), built and evaluated on the host in the device's order (test
 * hook; no device needed), as pd_atm_table; n_cells (may be NULL): its cells.  PD_ERR_UNSUPPORTED if
 * the builder's check is past 1e-14, where a handle would take the closed form. */
pd_status pd_atm_table_lds(const pd_params* params, const double* alt, int64_t n_alt, double* atm_out,
                           double* max_rel, int32_t* n_cells);
/* The wind profiles' interval slopes as those kernels' LDS image tabulates them (binary64): slope of
 * interval j of profile w at out[w][j], [PD_N_WIND_PROFILES][PD_MAX_WIND]; 0 past a profile's last
 * interval (test hook; no device needed). */
pd_status pd_wind_slopes(const pd_params* params, double* out);
/* Observation / action widths of the handle. */
int pd_obs_dim(const pd_env* env);
int pd_action_dim(const pd_env* env);

#ifdef __cplusplus
}
#endif
#endif
