/* mlmcpi_hip.h -- C ABI of the MI355X (gfx950) sweep engine.
 *
 * Drop-in boundary for the inner MCMC sweep of eikehmueller/mlmcpathintegral: every entry point
 * replaces the body of one virtual method of the reference's Action / Sampler / QoI interfaces
 * (cited per function, paths relative to the reference's src/), batched over B independent chains
 * that live in HBM.  Plain pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * Conventions
 *   - every function returns 0 on success, a negative mlmcpi_status otherwise;
 *     mlmcpi_last_error() gives the message of the calling thread's last failure;
 *   - pointers named d_* are DEVICE pointers (from mlmcpi_malloc or any HIP allocator, e.g. a
 *     torch tensor's data_ptr()); everything else is host memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls are
 *     asynchronous with respect to the host unless stated otherwise;
 *   - state layout is the reference's SampleState layout, chain-major:
 *       1-D paths      x[b*M + j]                         (common/samplestate.hh:19-53)
 *       GFF            phi[b*Mt*Mx + Mt*j + i]            (lattice/lattice2d.hh:230-245)
 *       Schwinger      theta[b*2*Mt*Mx + 2*Mt*j + 2*i + mu]  (lattice/lattice2d.hh:348-354)
 *       sigma model    phi[b*2*Mt*Mx + 2*(Mt*j + i) + {0: theta, 1: phi}]  (action/qft/nonlinearsigmaaction.hh:381-392)
 *   - randomness is counter based: Philox4x32-10 keyed by `seed`, counter =
 *     (site, chain0 + b, step, purpose<<24 | sub).  Results do not depend on grid shape, tile
 *     size, batch composition or number of GPUs -- to the last bit.
 *   - BIT REPRODUCIBILITY ACROSS LAUNCH PLANS holds for a FIXED (n_overrelax, fuse, MLMCPI_OR_KERNEL) setting only.
 *     The overrelaxation sweeps of one launch of the Schwinger action (mlmcpi_lattice_sweep_draw*) and of
 *     the rotor (mlmcpi_path_sweep_draw*) are evaluated as ONE closed form (K sweeps = one signed sum of
 *     2 K plaquettes / path differences per link / site): the same map as K single sweeps, other rounding.
 *     K sweeps in one launch and the same sweeps in two launches -- another `fuse`, or
 *     MLMCPI_OR_KERNEL=block (which makes BOTH actions sweep by sweep) -- differ in the last bits
 *     (<= 4e-14 Schwinger at K = 10, <= 2e-15 rotor).  A heat-bath accept/reject decision that sits on
 *     such a difference flips, after which two chains diverge: compare, checkpoint and resume runs under
 *     one launch plan, and record it (mlmcpi_lattice_sweep_plan: every launch of a draw, its kernel and depth K).  The
 *     sweep-by-sweep kernels (GFF and the sigma model always) agree bit for bit whatever the plan.  A QoI fused into the last launch of a
 *     draw (mlmcpi_lattice_sweep_draw_qoi*) sums per-tile partials in the tile order of that launch: under another plan
 *     (MLMCPI_OR_HEAT=split, MLMCPI_OR_KERNEL=block) it agrees to rounding (1e-13).  Spelled out in DESIGN.md 3 / 9.
 *   - CHAINS PER CALL.  B is the number of chains of one call; where the chains ride in the launch grid decides the largest B.
 *     The HIP runtime on the MI355X launches gridDim.y and gridDim.z beyond 65535 and every workgroup of such a grid runs with the
 *     right index (measured at 65535, 65536 and 65581 through mlmcpi_path_initialise: DESIGN.md "Chains per call"), so an entry
 *     point without a guard takes any B its buffers hold ("unbounded" below; batches whose element count B * n passes 2^32, 32 GB of
 *     state, have not been run and want an index audit first).  Four units refuse
 *     B > 65535 by name, with nothing launched; the guards are conservative and stay until someone needs them lifted.  Every entry
 *     point is run at B = 65535 and, where it takes it, at B = 65581 by tests/test_chain_count_gpu.py.
 *       entry points                                                                   chains ride on        largest B
 *       mlmcpi_path_evaluate / _force / _initialise, mlmcpi_qoi_xsquared /             grid y                unbounded
 *         _susceptibility, mlmcpi_path_copy_from_*, mlmcpi_path_hmc_draw
 *       mlmcpi_path_hmc_run                                                            grid x, 1 per         unbounded
 *                                                                                      workgroup (M a multiple of 64, <= 8192); else
 *                                                                                      grid y + x, 256 per workgroup
 *       mlmcpi_path_sweep_draw / _from / _qoi                                          grid y; QoI: x, 256   65535 (refused by name)
 *       mlmcpi_path_site_updates, mlmcpi_lattice_site_updates                          grid x, 64 per wg     unbounded
 *       mlmcpi_path_twolevel_draw / _masked                                            grid x, 1 per wg      unbounded
 *       mlmcpi_path_exact_draw                                                         grid y, 16 per row    unbounded
 *       mlmcpi_path_cluster_draw, mlmcpi_schwinger_cluster_*                           grid x, 4 per wg      unbounded
 *       mlmcpi_path_correlator, mlmcpi_schwinger_wilson_loops                          linear index, x then y 2^23 x 65535 workgroups
 *       mlmcpi_gff_correlator (its batch is spelled n_chains; run at the edge by       linear index, x then y unbounded (2^23 x 65535
 *         tests/test_gff_correlator_gpu.py)                                                                  workgroups)
 *       mlmcpi_lattice_evaluate / _force / _initialise / _sweep_draw* / _copy_from_* / grid y (finish kernels: unbounded
 *         _twolevel_draw* / _exact_draw / _hmc_draw, mlmcpi_qoi_phi_squared /          x, 4 or 1 per wg)
 *         _avg_plaquette / _2d_susceptibility / _magnetic_susceptibility
 *       mlmcpi_lattice_random_sweep_draw, mlmcpi_sigma_cluster_draw,                   grid x, 1 or more     unbounded
 *         mlmcpi_sigma_sw_draw, mlmcpi_sigma_level_cluster_* / _sw_*                   workgroups per chain
 *       mlmcpi_gff_level_evaluate / _draw, mlmcpi_gff_cfa_*                            grid x, 1 per wg      unbounded
 *       mlmcpi_gff_copy_from_*, mlmcpi_gff_twolevel_draw                               grid y                unbounded
 *       mlmcpi_sigma_level_initialise / _evaluate / _magnetic_susceptibility /         grid y                65535 (refused)
 *         _sweep_draw / _copy_from_*, mlmcpi_sigma_cfa_*, mlmcpi_sigma_twolevel_*
 *       mlmcpi_sigma_level_correlator                                                  grid y and z          65535 (refused by name)
 *       mlmcpi_sigma_level_topological_charge (its batch is spelled n_chains; run at   linear index, x then y unbounded (2^23 x 65535
 *         the edge by tests/test_sigma_topology_gpu.py)                                                      workgroups)
 *       mlmcpi_sigma_level_cooled_charge (n_chains; run at the edge by                 linear index, x then y unbounded (2^23 x 65535
 *         tests/test_sigma_cooling_gpu.py)                                                                   workgroups)
 *       mlmcpi_sigma_level_flowed_charge (n_chains; run at the edge by                 linear index, x then y unbounded (2^23 x 65535
 *         tests/test_sigma_flow_gpu.py)                                                                      workgroups)
 *       mlmcpi_stats_accumulate, mlmcpi_stats_window_record                            grid x, 256 per wg    unbounded
 */
#ifndef MLMCPI_HIP_H
#define MLMCPI_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLMCPI_ABI_VERSION 1

enum mlmcpi_status {
  MLMCPI_OK = 0,
  MLMCPI_ERR_INVALID = -1,     /* bad argument (sizes, parity, NULL pointers) */
  MLMCPI_ERR_HIP = -2,         /* HIP runtime error, see mlmcpi_last_error() */
  MLMCPI_ERR_UNSUPPORTED = -3, /* operation not defined for this action (action/action.hh:73-96) */
  MLMCPI_ERR_NO_DEVICE = -4
};

/* action kinds */
enum mlmcpi_action_kind {
  MLMCPI_HARMONIC = 0,  /* action/qm/harmonicoscillatoraction.{hh,cc} */
  MLMCPI_QUARTIC = 1,   /* action/qm/quarticoscillatoraction.{hh,cc} */
  MLMCPI_ROTOR = 2,     /* action/qm/rotoraction.{hh,cc} */
  MLMCPI_GFF = 3,       /* action/qft/gffaction.{hh,cc} (n_gibbs_smooth = 0) */
  MLMCPI_SCHWINGER = 4, /* action/qft/quenchedschwingeraction.{hh,cc} */
  MLMCPI_NONLINEAR_SIGMA = 5 /* action/qft/nonlinearsigmaaction.{hh,cc}: O(3) spins as (theta, phi) per vertex; uses `beta`.
                              * Through mlmcpi_lattice_*: sweeps, evaluate, force, initialise, site updates and QoI 4 on the
                              * unrotated lattice; NOT HMC (the reference's force samples exp(-S) dtheta dphi, without the sin
                              * theta of the measure), and NOT mlmcpi_lattice_copy_from_* / mlmcpi_lattice_twolevel_*, whose
                              * (rt, rx) describe unrotated coarsenings: MLMCPI_ERR_UNSUPPORTED.  The action coarsens by
                              * CoarsenRotate only (nonlinearsigmaaction.hh:143-149); its rotated levels, the transfers, the
                              * conditioned fine action and the two-level step are mlmcpi_sigma_level_* / mlmcpi_sigma_cfa_* /
                              * mlmcpi_sigma_twolevel_* below.  Sweeps are bit-identical whatever
                              * the launch plan: every update reads spins recomputed from the stored angles. */
};

/* 1-D path action: lattice/lattice1d.hh:60-101 (M_lat, T_final, a = T_final/M_lat) + the action's
 * own parameters (m0, mu2; lambda, x0 for the quartic oscillator). */
typedef struct mlmcpi_path_action {
  int32_t kind;
  uint32_t M;
  double T_final, m0, mu2, lambda, x0;
} mlmcpi_path_action;

/* 2-D lattice action on an unrotated Mt x Mx periodic lattice (lattice/lattice2d.hh:98-437).
 * GFF uses `mass` (mu2 = (mass/Mt)^2, action/qft/gffaction.hh:174-181); Schwinger and the sigma model use `beta`. */
typedef struct mlmcpi_lattice_action {
  int32_t kind;
  uint32_t Mt, Mx;
  double beta, mass;
} mlmcpi_lattice_action;

/* ---- runtime plumbing ---------------------------------------------------------------------- */
int mlmcpi_abi_version(void);
const char *mlmcpi_last_error(void);
int mlmcpi_device_count(int *count);
int mlmcpi_set_device(int device);
int mlmcpi_device_name(char *buf, size_t len);
int mlmcpi_malloc(void **d_ptr, size_t bytes);
int mlmcpi_free(void *d_ptr);
int mlmcpi_memset(void *d_ptr, int value, size_t bytes, void *stream);
int mlmcpi_copy_h2d(void *d_dst, const void *src, size_t bytes, void *stream);
int mlmcpi_copy_d2h(void *dst, const void *d_src, size_t bytes, void *stream);
int mlmcpi_copy_d2d(void *d_dst, const void *d_src, size_t bytes, void *stream);
int mlmcpi_stream_synchronize(void *stream);
/* Tuning knobs -- they change no result beyond the last bits.  Read from the environment once, at the first use in the
 * process; this call changes one afterwards (value "" or NULL resets it): MLMCPI_SWEEP_TILE=TWxTHxNT (tile and workgroup
 * size of the generic sweep kernels; also forces them), MLMCPI_OR_KERNEL=perm|block (Schwinger overrelaxation in closed
 * form -- the default on even lattices of at least 64 x 32 -- or sweep by sweep on 4 x 4 register blocks where 64 x 64
 * tiles divide the lattice, the generic kernels elsewhere, with the heat-bath sweep in a launch of its own; the
 * sweep-by-sweep kernels agree with each other bit for bit and with the closed form to 4e-14), MLMCPI_OR_HEAT=
 * fused|split|wide|narrow (the heat-bath sweep behind the last overrelaxation launch: in it or in a launch of its own;
 * workgroup size of the fused launch). */
int mlmcpi_set_option(const char *name, const char *value);

/* ---- index maps (host, integer, bit-exact) --------------------------------------------------
 * lattice/lattice2d.hh:230-268 (vertex), :348-375 (link); rotated != 0 selects the 45-degree
 * sublattice numbering. */
uint32_t mlmcpi_vertex_cart2lin(uint32_t Mt, uint32_t Mx, int rotated, int i, int j);
void mlmcpi_vertex_lin2cart(uint32_t Mt, uint32_t Mx, int rotated, uint32_t ell, int *i, int *j);
uint32_t mlmcpi_link_cart2lin(uint32_t Mt, uint32_t Mx, int i, int j, int mu);
void mlmcpi_link_lin2cart(uint32_t Mt, uint32_t Mx, uint32_t ell, int *i, int *j, int *mu);
/* neighbour tables as the Lattice constructors build them: lattice/lattice1d.cc:11-18 (M x 2),
 * lattice/lattice2d.cc:137-155 (nvertices x 8; +i,-i,+j,-j then the four diagonals) */
int mlmcpi_neighbours_1d(uint32_t M, uint32_t *out);
int mlmcpi_neighbours_2d(uint32_t Mt, uint32_t Mx, int rotated, uint32_t *out);

/* ---- 1-D paths ------------------------------------------------------------------------------ */
/* Action::evaluate (action/action.hh:60-61): d_S[b] = S[x_b]. */
int mlmcpi_path_evaluate(const mlmcpi_path_action *act, const double *d_x, uint32_t B, double *d_S, void *stream);
/* Action::force (action/action.hh:112-113): d_f[b*M+j] = dS/dx_j. */
int mlmcpi_path_force(const mlmcpi_path_action *act, const double *d_x, double *d_f, uint32_t B, void *stream);
/* Action::initialise_state (action/action.hh:122-123): rotor U(-pi,pi) per site
 * (rotoraction.cc:82-89), zeros for HO / quartic. */
int mlmcpi_path_initialise(const mlmcpi_path_action *act, double *d_x, uint32_t B, uint64_t seed, uint32_t chain0,
                           void *stream);
/* QoIXsquared::evaluate (qoi/qm/qoixsquared.cc:7-20) and QoISusceptibility::evaluate
 * (qoi/qm/qoisusceptibility.cc:8-23); d_out[b]. */
int mlmcpi_qoi_xsquared(const double *d_x, uint32_t M, uint32_t B, double *d_out, void *stream);
int mlmcpi_qoi_susceptibility(const double *d_x, uint32_t M, double T_final, uint32_t B, double *d_out,
                              void *stream);

/* HMCSampler::draw (sampler/hmcsampler.cc:8-19) = n_rep x single_step (:22-69), fused: momenta,
 * nt+1 force evaluations, both action evaluations, kinetic energies and the global Metropolis
 * test run on the device; momenta never touch HBM.  Repetition r of this call uses Philox step
 * traj0 + r; as in the reference, repetitions after the first acceptance are skipped.
 *   d_x        [B*M]  current states, updated in place where accepted
 *   d_work     workspace of mlmcpi_path_hmc_workspace_bytes() bytes
 *   d_accept   [B] int32, 1 where the draw was accepted (MCMCStep::accepted, mcmcstep.hh:47)
 *   d_energies optional [B*4]: S(x_cur), T(p_0), S(x_trial), T(p_end) of the last repetition run */
int mlmcpi_path_hmc_workspace_bytes(const mlmcpi_path_action *act, uint32_t B, uint32_t nt, size_t *bytes);
int mlmcpi_path_hmc_draw(const mlmcpi_path_action *act, double *d_x, uint32_t B, uint32_t nt, double dt,
                         uint32_t n_rep, uint64_t seed, uint32_t chain0, uint32_t traj0, void *d_work,
                         int32_t *d_accept, double *d_energies, void *stream);

/* n_draws consecutive HMCSampler::draw calls, each followed by a QoI evaluation -- the body of the loop
 * of MonteCarloSingleLevel::evaluate (montecarlo/montecarlosinglelevel.cc:59-77) -- without returning
 * to the host: for paths that fit one workgroup (M <= 8192, multiple of 64) everything, including the
 * Metropolis tests and the QoIs, runs in ONE launch with the state in registers throughout.  Results equal
 * n_draws x (mlmcpi_path_hmc_draw with traj0 + d*n_rep, then the QoI kernel) up to fp contraction.
 *   qoi_kind  0 none, 1 QoIXsquared, 2 QoISusceptibility;  d_qoi [B*n_draws] (chain-major) for the
 *   one-launch path, [n_draws*B] (draw-major) for segmented paths -- see mlmcpi_path_hmc_run_layout();
 *   d_accept_count [B] int32 (optional): accepted draws per chain. */
int mlmcpi_path_hmc_run(const mlmcpi_path_action *act, double *d_x, uint32_t B, uint32_t nt, double dt, uint32_t n_rep,
                        uint32_t n_draws, int qoi_kind, uint64_t seed, uint32_t chain0, uint32_t traj0, void *d_work,
                        double *d_qoi, int32_t *d_accept_count, void *stream);
/* 1 if d_qoi of mlmcpi_path_hmc_run is chain-major [B][n_draws] for this action / nt, 0 if draw-major */
int mlmcpi_path_hmc_run_layout(const mlmcpi_path_action *act, uint32_t B, uint32_t nt, int32_t *chain_major);
/* The launch geometry the three calls above choose from (kind, M, B, nt); host only, no device is touched.  NT threads hold
 * R consecutive sites each.  halo == 0: one workgroup holds the whole periodic path in registers (NT * R == M, nseg == 1,
 * owned_len == M) and mlmcpi_path_hmc_run is one launch (chain_major == 1, what mlmcpi_path_hmc_run_layout reports).
 * Otherwise segment s of nseg owns the sites [s * owned_len, min(M, (s + 1) * owned_len)) in the middle of a buffer of NT * R
 * sites whose first and last halo = nt + 1 sites are recomputed copies of the neighbouring segments.  An nt too long for the
 * buffer (2 halo + 64 > NT * R) is MLMCPI_ERR_INVALID here as in the calls above. */
typedef struct mlmcpi_path_hmc_plan_info {
  uint32_t R, NT, nseg, owned_len, halo;
  int32_t chain_major;
} mlmcpi_path_hmc_plan_info;
int mlmcpi_path_hmc_plan(const mlmcpi_path_action *act, uint32_t B, uint32_t nt, mlmcpi_path_hmc_plan_info *out);

/* The time correlator of a path (path_correlator.hip): per chain b of d_x [B][M], for tau = 0 .. n_lag - 1,
 *   kinds 0, 1 (oscillators)  C(tau) = (1/M) sum_j x_j x_{(j + tau) mod M}
 *   kind 2 (rotor)            C(tau) = (1/M) sum_j cos(x_j - x_{(j + tau) mod M}), formed as c_j c_{j+tau} + s_j s_{j+tau} from one
 *                             sincos per staged site
 * into d_out [B][n_lag].  Only act->kind and act->M are read.  n_lag <= M/2 + 1: C(M - tau) = C(tau).
 * Identities: C(0) = QoIXsquared (oscillators), C(0) = 1 (rotor); with w(0) = 1, w(M/2) = 1 for even M and w = 2 otherwise (M = 2:
 * both lags weight 1; odd M: every lag but 0 weight 2), sum_{tau <= M/2} w C(tau) = (sum_j x_j)^2 / M for the oscillators and
 * ((sum_j c_j)^2 + (sum_j s_j)^2) / M for the rotor.  The decay of <C(tau)> gives the gap: m_eff(tau) = acosh((C(tau - 1) + C(tau + 1)) /
 * (2 C(tau))) = a (E_1 - E_0) where one state dominates (include/mlmcpi/correlator.hh has the lattice closed forms).
 * Summation order: sites and lags go in tiles of J = 8 sites and T = 8 lags.  A path is cut into nseg segments of `owned` sites
 * (a multiple of 8 but for the last; nseg = 1 while the path's tiles and the lag tiles fit one LDS image of 64 KiB).  For a
 * segment and a lag, a group of G lanes (G = min(64, owned tiles rounded up to a power of two)) adds: lane g the site tiles g, g +
 * G, .. ascending, sites ascending in a tile, one FMA per product (rotor: the c product, then the s product, of each site); the lanes
 * by the shuffle tree, offsets G/2, .., 1.  Segments are added in ascending order; the sum is divided by M last.  The geometry is a
 * function of (kind, M, n_lag) alone, there are no atomics and no tuning knob: a chain's output is the same bits for every B, every
 * split of the chains over calls and every stream.
 * n_lag cap: the LDS image of a segment holds tiles of 8 sites, 80 bytes each per component, the lag tiles beside at least one site
 * tile: ceil(n_lag / 8) + 1 <= 65536 / (80 components), i.e. n_lag <= 6544 for the oscillators and <= 3264 for the rotor; beyond:
 * MLMCPI_ERR_UNSUPPORTED.
 * d_acc (may be NULL) [B][n_lag][2]: C is ADDED to [.][.][0] and C^2 to [.][.][1] in the launch that writes d_out; the caller
 * counts the calls.  d_work: _workspace_bytes(act, n_lag, B) bytes (never 0), 256-byte aligned; content at entry ignored.
 * Chains and segments share one index of workgroups, ceil(B / chains_per_workgroup) nseg of them, laid over grid x (2^31 / 256) and,
 * beyond that, y: there is no 65535-chain limit (the bound, 2^23 x 65535 workgroups, is beyond any memory; CHAINS PER CALL above).
 * MLMCPI_ERR_INVALID, with nothing launched and no output byte touched: NULL act, d_x, d_out or d_work; kind outside 0 .. 2; M = 0,
 * B = 0 or n_lag = 0; n_lag > M/2 + 1; more workgroups than above; work_bytes below _workspace_bytes.
 * _plan (host only, touches no device) reports the geometry and returns the status the call would. */
typedef struct mlmcpi_path_correlator_plan_info {
  uint64_t work_bytes;            /* what _workspace_bytes reports */
  uint64_t grid;                  /* workgroups of the correlator launch; with work_bytes the only entries that depend on B */
  uint32_t workgroup;             /* threads of a workgroup */
  uint32_t chains_per_workgroup;  /* 4 (short paths: one wave per chain) or 1 */
  uint32_t waves_per_chain;       /* 1 or 4 */
  uint32_t group;                 /* G: lanes that share a lag tile */
  uint32_t owned;                 /* sites a segment owns: segment s owns [s owned, min(M, (s + 1) owned)) */
  uint32_t nseg;
  uint32_t J, T;                  /* sites x lags of a lane's register tile */
  uint32_t lag_tiles;             /* ceil(n_lag / T): lag tile q holds the lags [q T, min(n_lag, (q + 1) T)) */
  uint32_t image_tiles;           /* tiles of J sites in a segment's LDS image: owned tiles + lag_tiles */
  uint32_t components;            /* 1, rotor 2 */
  uint32_t lds_bytes, lds_limit;  /* dynamic LDS of a workgroup, and the limit the kernel is written for */
} mlmcpi_path_correlator_plan_info;
int mlmcpi_path_correlator_workspace_bytes(const mlmcpi_path_action *act, uint32_t n_lag, uint32_t B, size_t *bytes);
int mlmcpi_path_correlator(const mlmcpi_path_action *act, const double *d_x, uint32_t B, uint32_t n_lag, double *d_out /* [B][n_lag] */,
                           double *d_acc /* [B][n_lag][2], may be NULL */, void *d_work, size_t work_bytes, void *stream);
int mlmcpi_path_correlator_plan(const mlmcpi_path_action *act, uint32_t n_lag, uint32_t B, mlmcpi_path_correlator_plan_info *out);

/* OverrelaxedHeatBathSampler::draw (sampler/overrelaxedheatbathsampler.cc:8-31) for the rotor:
 * n_overrelax sweeps of RotorAction::overrelaxation_update (rotoraction.cc:40-56) then n_heatbath
 * sweeps of heatbath_update (:20-37), even sites then odd sites within each sweep.  Sweep s of
 * this call uses Philox step sweep0 + s.  d_x is updated in place; d_scratch is B*M doubles.
 * At most 65535 chains per call (they are one grid dimension of every launch; _from and _qoi too): more is an error (the
 * table under CHAINS PER CALL at the top of this header).
 * Up to 16 overrelaxation sweeps of a launch are applied in closed form (more: launches of equal depth);
 * MLMCPI_OR_KERNEL=block sweeps one by one, 8 per launch.  The two agree to <= 2e-15 without a heat bath
 * behind (the same map, other rounding), NOT bit for bit: see "bit reproducibility across launch plans"
 * at the top of this header. */
int mlmcpi_path_sweep_draw(const mlmcpi_path_action *act, double *d_x, double *d_scratch, uint32_t B,
                           uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0,
                           uint32_t sweep0, void *stream);

/* The same with the input left untouched (see mlmcpi_lattice_sweep_draw_from): reads d_src, alternates between d_w0 and
 * d_w1 (which may equal d_src), *result_in = 0 / 1 names the buffer holding the result; no final copy. */
int mlmcpi_path_sweep_draw_from(const mlmcpi_path_action *act, const double *d_src, double *d_w0, double *d_w1, uint32_t B,
                                uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0, uint32_t sweep0,
                                int32_t *result_in, void *stream);
/* mlmcpi_path_sweep_draw_from with the topological susceptibility of the new sample (QoISusceptibility,
 * qoi/qm/qoisusceptibility.cc:8-23: chi = Q^2 / T, Q = sum_j mod_2pi(x_j - x_{j-1}) / 2 pi) summed inside the draw's last
 * launch, while the segments are in LDS: d_qoi[b]; and, with d_acc != NULL, stats->record_sample of it into d_acc[B][5] in
 * the same call (mlmcpi_stats_accumulate's recurrence): one pass of the loop at montecarlo/montecarlosinglelevel.cc:59-77.
 * Same value as mlmcpi_qoi_susceptibility on the result up to the order of the summation. */
int mlmcpi_path_sweep_draw_qoi(const mlmcpi_path_action *act, const double *d_src, double *d_w0, double *d_w1, uint32_t B,
                               uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0, uint32_t sweep0,
                               double *d_qoi, double *d_acc, int32_t *result_in, void *stream);

/* Action::heatbath_update / overrelaxation_update(state, l) (action/action.hh:73-96; rotoraction.cc:20-56): the update of
 * site l for every chain of the batch -- of the n sites d_sites[0 .. n) (device memory) in list order when d_sites is not
 * NULL, of the single site `site` otherwise.  One thread per chain walks the list, so the updates are sequential within
 * a chain exactly as in the reference's loops (overrelaxedheatbathsampler.cc:8-31: lexicographic or shuffled index
 * sets); chains run in parallel.  heat != 0: heat bath, else overrelaxation.  Random numbers: Philox (site, chain,
 * step), the sweeps' contract, so the sites of one colour visited with a sweep's step reproduce that phase of the sweep.
 * This is the reference's CPU inner loop kept for callers that walk index sets themselves; the fast path is a sweep. */
int mlmcpi_path_site_updates(const mlmcpi_path_action *act, double *d_x, uint32_t B, const uint32_t *d_sites, uint32_t n,
                             uint32_t site, int32_t heat, uint64_t seed, uint32_t chain0, uint32_t step, void *stream);

/* TwoLevelMetropolisStep::draw (montecarlo/twolevelmetropolisstep.cc:35-89) with QMAction::copy_from_{coarse,fine}
 * (action/qm/qmaction.cc:7-24) and the action's conditioned fine action: Gaussian for the harmonic / quartic
 * oscillator (action/qm/gaussianconditionedfineaction.cc:7-43), ExpSin2 for the rotor
 * (action/qm/rotorconditionedfineaction.cc:7-43; theta'[2j+1] = mod_2pi(Wmin + ExpSin2(2 W''))):
 *   theta'[2j] = x_coarse[j];  theta'[2j+1] ~ N(Wmin(theta'[2j], theta'[2j+2]), 1/W'')
 *   dS = [S_f(theta') - S_f(theta)] + [S_c(theta_C) - S_c(x_coarse)] + [S_cfa(theta) - S_cfa(theta')]
 *   accept with min(1, exp(-dS)); accepted chains get theta <- theta'.
 * `fine` lives on M sites, `coarse` on M/2 (its parameters are the caller's: same as fine for the quartic
 * oscillator, renormalised or not for the HO).  d_theta [B*M] is the step's current fine state
 * (MCMCStep::set_state), d_x_coarse [B*M/2] the coarse-level proposal.  d_terms (optional, [B*3]) receives
 * the three action differences.  Philox step = `step`. */
int mlmcpi_path_twolevel_workspace_bytes(const mlmcpi_path_action *fine, uint32_t B, size_t *bytes);
int mlmcpi_path_twolevel_draw(const mlmcpi_path_action *fine, const mlmcpi_path_action *coarse, const double *d_x_coarse,
                              double *d_theta, uint32_t B, uint64_t seed, uint32_t chain0, uint32_t step, void *d_work,
                              int32_t *d_accept, double *d_terms, void *stream);

/* The same with a per-chain mask (d_mask may be NULL = all ones; d_mask may be the d_accept of the level below): chains
 * with d_mask[b] == 0 are left alone -- d_accept[b] = 0, d_theta[b] untouched, no random numbers of the step consumed for
 * them.  This is the `if (not accept) break` of HierarchicalSampler::draw (sampler/hierarchicalsampler.cc:62-76) for a
 * batch of chains: a chain whose move was rejected on a coarser level does not move on the finer ones. */
int mlmcpi_path_twolevel_draw_masked(const mlmcpi_path_action *fine, const mlmcpi_path_action *coarse, const double *d_x_coarse,
                                     double *d_theta, uint32_t B, uint64_t seed, uint32_t chain0, uint32_t step, void *d_work,
                                     const int32_t *d_mask, int32_t *d_accept, double *d_terms, void *stream);

/* QMAction::copy_from_fine / copy_from_coarse (action/qm/qmaction.cc:7-24): coarse[j] <-> fine[2j]; the odd
 * fine sites are left untouched.  d_fine [B*2*M_coarse], d_coarse [B*M_coarse]. */
int mlmcpi_path_copy_from_fine(const double *d_fine, double *d_coarse, uint32_t M_coarse, uint32_t B, void *stream);
int mlmcpi_path_copy_from_coarse(const double *d_coarse, double *d_fine, uint32_t M_coarse, uint32_t B, void *stream);
/* Exact sampler of the harmonic oscillator (the action is its own Sampler in the reference).
 * mlmcpi_ho_cholesky_factor: HarmonicOscillatorAction::build_covariance (action/qm/harmonicoscillatoraction.cc:38-56)
 *   on the host: lower Cholesky factor L of the covariance = inverse of the circulant precision matrix, O(M^3);
 *   h_LT [M][M] (host memory) receives L^T row-major, h_LT[k*M + j] = L[j][k].  M_lat <= 4096.
 * mlmcpi_path_exact_draw: HarmonicOscillatorAction::draw (:59-66): d_x[b] = L y[b], y ~ N(0,1)^M from Philox
 *   (entries 2m, 2m+1 = the Box-Muller pair of site m, purpose P_EXACT, step `step`), for B chains -- a dense
 *   [B x M] . [M x M] fp64 product on the matrix cores.  d_LT = h_LT copied to the device. */
int mlmcpi_ho_cholesky_factor(const mlmcpi_path_action *act, double *h_LT);
int mlmcpi_path_exact_draw(const mlmcpi_path_action *act, const double *d_LT, double *d_x, uint32_t B, uint64_t seed,
                           uint32_t chain0, uint32_t step, void *stream);

/* ClusterSampler::draw on a 1-D lattice (sampler/clustersampler.cc:36-49, single_cluster_update1d :92-132, with
 * RotorAction::new_reflection / S_ell / flip, action/qm/rotoraction.hh:226-253): n_updates reflection-cluster updates of
 * every chain, in place, one launch.  MLMCPI_ROTOR only; MLMCPI_ERR_UNSUPPORTED for the oscillators (no reflection symmetry
 * of the bond form).  Update k of this call has the counter update0 + k: xbar = 2 pi u - pi and the seed site
 * i0 = min(floor(v M), M - 1) from Philox (site 0, purpose 15); link l = (l, l + 1 mod M) is bonded iff its uniform (site
 * l >> 1, purpose 16: u for l even, v for l odd) < 1 - exp(min(0, -(2 m0 / a) cos(x_l - xbar) cos(x_{l+1} - xbar))) on the
 * path BEFORE the update; the run of bonded links around i0 is reflected, x <- mod_2pi(pi + 2 xbar - x).  A run that
 * reaches all M sites flips all M once (the reference's walk re-tests the link into its own seed there: DESIGN.md 5).
 * Ten updates in one call equal 5 + 5; results do not depend on the batch split.
 *   d_cluster_sites  optional [B] uint32: the flipped sites of this call's updates are ADDED to it, per chain (the caller
 *                    zeroes it when it wants the count of one call; 32 bits: a caller that lets it run must read and zero
 *                    it before 2^32 flipped sites per chain).  update0 + n_updates must fit 32 bits: MLMCPI_ERR_INVALID. */
int mlmcpi_path_cluster_draw(const mlmcpi_path_action *act, double *d_x, uint32_t B, uint32_t n_updates, uint64_t seed,
                             uint32_t chain0, uint32_t update0, uint32_t *d_cluster_sites, void *stream);

/* ---- 2-D lattices --------------------------------------------------------------------------- */
/* QuenchedSchwingerClusterSampler (sampler/quenchedschwingerclustersampler.{hh,cc}).  The sampler's state is a closed path
 * d_psi [B][Mt Mx] of plaquette angles, a rotor with m0 / a = beta (:19-26); the link field is rebuilt from it on every draw.
 *   _init   RotorAction::initialise_state of the path (U(-pi, pi) per site)
 *   _draw   :40-86: n_updates cluster updates of d_psi (update counters draw0 n_updates + k), then the rebuild with the
 *           gauge transformation of draw `draw0`; d_theta [B][2 Mt Mx] is overwritten, its previous content ignored;
 *           d_work: _workspace_bytes, zeroed by the caller once (uint32 [B]: flipped sites per chain, added up over the draws)
 *   _links  the rebuild alone: theta_1(i, j) = sum_{i' < i} (psi[i' Mx + j + 1] - psi[i' Mx + j]), theta_0 = 0 except row
 *           Mt - 1, theta_0(Mt - 1, j) = -sum_{i'} (psi[i' Mx + j] - psi[i' Mx]) (the closed form of :52-68), then
 *           theta_0(i, j) += g(i, j) - g(i + 1, j), theta_1(i, j) += g(i, j) - g(i, j + 1) with one uniform angle per vertex
 *           (Philox site (Mt j + i) >> 1, purpose 17, step draw0; gauge = 0: g = 0) and mod_2pi.  The plaquette of cell
 *           c = i Mx + j is mod_2pi(psi[c + 1] - psi[c]), psi[Mt Mx] = psi[0].
 * MLMCPI_SCHWINGER only: MLMCPI_ERR_UNSUPPORTED otherwise (the sigma model's generic 2-D cluster update is not implemented). */
int mlmcpi_schwinger_cluster_workspace_bytes(const mlmcpi_lattice_action *act, uint32_t B, size_t *bytes);
int mlmcpi_schwinger_cluster_init(const mlmcpi_lattice_action *act, double *d_psi, uint32_t B, uint64_t seed, uint32_t chain0,
                                  void *stream);
int mlmcpi_schwinger_cluster_draw(const mlmcpi_lattice_action *act, double *d_psi, double *d_theta, uint32_t B,
                                  uint32_t n_updates, uint64_t seed, uint32_t chain0, uint32_t draw0, double *d_work,
                                  void *stream);
int mlmcpi_schwinger_cluster_links(const mlmcpi_lattice_action *act, const double *d_psi, double *d_theta, uint32_t B, int gauge,
                                   uint64_t seed, uint32_t chain0, uint32_t draw0, void *stream);
/* Wolff single-cluster update of the O(3) nonlinear sigma model (sigma_cluster.hip): n_updates updates of
 * every chain of d_phi [B][2 Mt Mx], in place, one launch.  NOT the reference's ClusterSampler for this action, whose walk
 * bonds the four diagonal neighbours as well and samples another model: this is that walk over the four links
 * per vertex the action couples.  Vertex l = Mt j + i; link (l, 0) joins l to its +i neighbour, link (l, 1) to its +j
 * neighbour (periodic; on an extent of 2 the two links between a pair of vertices are two links).  Update k of this call
 * has the counter update0 + k: Philox (site 0, purpose 19) sub 0 (u, v) -> the reflection normal r, r_z = 1 - 2 u, azimuth
 * 2 pi v - pi; sub 1 u -> the seed vertex min(floor(u N), N - 1).  With a_l = r . sigma_l of the field BEFORE the update, link
 * (x, y) is bonded iff its uniform (site l, purpose 20: u for link (l, 0), v for link (l, 1)) < 1 - exp(min(0, -2 beta
 * (a_x a_y))).  Every vertex of the connected component of the seed is reflected once, sigma' = sigma - 2 a r, and stored in
 * the canonical form theta = atan2(sqrt(sx^2 + sy^2), sz), phi = atan2(sy, sx).  Ten updates in one call equal 5 + 5;
 * results do not depend on the batch split, chain0, the launch plan or the order of the traversal.
 *   d_cluster_sites  optional [B] uint32: the flipped sites of this call's updates are ADDED to it, per chain (32 bits, as
 *                    for mlmcpi_path_cluster_draw: it wraps, also inside one call when n_updates Mt Mx >= 2^32; a caller
 *                    that wants exact counts keeps n_updates Mt Mx below that and reads and zeroes it in time)
 *   d_work           _workspace_bytes (12 B per vertex and chain for the queue, 1 bit for the membership map); its content
 *                    at entry is ignored
 * MLMCPI_NONLINEAR_SIGMA only: MLMCPI_ERR_UNSUPPORTED otherwise.  Any lattice of the sigma sweep (and odd extents): Mt, Mx >= 2,
 * Mt Mx <= 2^30.  update0 + n_updates must fit 32 bits: MLMCPI_ERR_INVALID. */
int mlmcpi_sigma_cluster_workspace_bytes(const mlmcpi_lattice_action *act, uint32_t B, size_t *bytes);
int mlmcpi_sigma_cluster_draw(const mlmcpi_lattice_action *act, double *d_phi, uint32_t B, uint32_t n_updates, uint64_t seed,
                              uint32_t chain0, uint32_t update0, uint32_t *d_cluster_sites, void *d_work, void *stream);
/* Swendsen-Wang multi-cluster update of the O(3) nonlinear sigma model (sigma_sw.hip): n_updates updates of
 * every chain of d_phi [B][2 Mt Mx], in place.  The multi-cluster form of the embedding of mlmcpi_sigma_cluster_draw, the
 * project's own sampler (the reference has none): one update tests all 2 N links once, labels every connected component of
 * the bonded links and reflects each component with probability 1/2.  Vertex l = Mt j + i; link (l, 0) joins l to its +i
 * neighbour, link (l, 1) to its +j neighbour (periodic; on an extent of 2 the two links between a pair of vertices are two
 * links with a uniform each).  Update k of this call has the counter update0 + k.  Philox purposes: 21, site 0, sub 0: (u, v)
 * -> the reflection normal r, r_z = 1 - 2 u, azimuth 2 pi v - pi; 22, site l, sub 0: u decides link (l, 0), v link (l, 1):
 * with a_l = r . sigma_l of the field BEFORE the update a link (x, y) is bonded iff a_x a_y > 0 and its uniform < 1 - exp(min(0,
 * -2 beta (a_x a_y))) (the product first); 23, site = the root of a cluster = its smallest vertex index, sub 0: the cluster
 * is reflected iff u < 0.5 (a vertex without a bond is a cluster of one and takes its own coin).  Every vertex of a reflected
 * cluster becomes sigma' = sigma - 2 a r, stored in the canonical form theta = atan2(sqrt(sx^2 + sy^2), sz), phi = atan2(sy,
 * sx).  Every decision is a function of (link or root, global chain index, counter, field before the update): the state is
 * bit-identical under every launch plan, tile size, batch split and chain0, and ten updates in one call equal 5 + 5.
 * Outputs, each an optional [B] array that is ADDED to, per chain:
 *   d_flipped   uint32: the vertices this call's updates reflected (32 bits: it wraps)
 *   d_clusters  uint32: the clusters of this call's updates (roots; 32 bits: it wraps)
 *   d_improved  double: per update 3 sum_C A_C^2 / N, A_C = sum of a_l over cluster C, an unbiased estimator of chi_m =
 *               <|M|^2> / N evaluated on the field before the update; A_C is summed in 64-bit fixed point (llrint(a 2^32),
 *               integer atomics) and the squares over the roots in one reduction of fixed configuration, so the value does not
 *               depend on the launch plan; it is added update by update, so 10 updates equal 5 + 5 to the bit
 *   d_work      _workspace_bytes (21 B per vertex and chain + 256 B); its content at entry is ignored
 * The call returns after its launches have finished: it reads back the status word the labelling loops set if one of them
 * ran into its iteration cap (MLMCPI_ERR_HIP; it cannot by construction, and it is an error, not a hang).
 * MLMCPI_NONLINEAR_SIGMA only: MLMCPI_ERR_UNSUPPORTED otherwise, and when MLMCPI_SIGMA_SW_PLAN=chain is forced on a lattice
 * beyond that plan's LDS bound.  MLMCPI_ERR_INVALID: Mt or Mx < 2, Mt Mx > 2^30, no workspace, update0 + n_updates beyond 32
 * bits. */
int mlmcpi_sigma_sw_workspace_bytes(const mlmcpi_lattice_action *act, uint32_t B, size_t *bytes);
int mlmcpi_sigma_sw_draw(const mlmcpi_lattice_action *act, double *d_phi, uint32_t B, uint32_t n_updates, uint64_t seed,
                         uint32_t chain0, uint32_t update0, uint32_t *d_flipped, uint32_t *d_clusters, double *d_improved,
                         void *d_work, void *stream);
int mlmcpi_lattice_state_size(const mlmcpi_lattice_action *act, uint32_t *n); /* Action::sample_size */
int mlmcpi_lattice_evaluate(const mlmcpi_lattice_action *act, const double *d_phi, uint32_t B, double *d_S,
                            void *stream);
int mlmcpi_lattice_force(const mlmcpi_lattice_action *act, const double *d_phi, double *d_f, uint32_t B,
                         void *stream);
/* Schwinger: U(-pi,pi) per link (quenchedschwingeraction.cc:198-204).  Sigma model: uniform on the sphere
 * (nonlinearsigmaaction.cc:141-162), cos theta = 1 - 2u, phi = 2 pi u' - pi from the uniforms of entries 2l, 2l + 1.  GFF: an exact draw from the action's
 * distribution, as in the reference (gffaction.cc:121-123: initialise_state = draw) -- by spectral synthesis
 * (see mlmcpi_lattice_exact_draw; its own Philox sub-stream) instead of the reference's sparse Cholesky solve. */
int mlmcpi_lattice_initialise(const mlmcpi_lattice_action *act, double *d_phi, uint32_t B, uint64_t seed,
                              uint32_t chain0, void *stream);
/* OverrelaxedHeatBathSampler::draw on a 2-D action: n_overrelax overrelaxation sweeps then
 * n_heatbath heat-bath sweeps (gffaction.cc:33-42,68-77; quenchedschwingeraction.cc:25-65 with
 * distribution/expcosdistribution.hh:51-65), multicolour order (GFF: (i+j) even, odd; Schwinger:
 * mu=0 & j even, mu=0 & j odd, mu=1 & i even, mu=1 & i odd; sigma model: nonlinearsigmaaction.cc:24-91, (i+j) even,
 * odd, heat bath by one Philox call of purpose 14 per vertex).  Mt and Mx must be even.  Sweep s
 * uses Philox step sweep0 + s.  d_phi is updated in place; d_scratch has the same size.
 * `fuse` = max number of consecutive overrelaxation sweeps fused into one launch (0 = library default: Schwinger closed
 * form 10; register-block kernels 6, in launches of equal depth, on lattices that 64 x 64 tiles divide; 4 otherwise.  The
 * heat-bath sweep behind the last overrelaxation launch rides in it where the fused kernels apply, else it gets a launch
 * of its own); results do not depend on it beyond the last bits of the Schwinger closed form (see the contract above). */
int mlmcpi_lattice_sweep_draw(const mlmcpi_lattice_action *act, double *d_phi, double *d_scratch, uint32_t B,
                              uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0,
                              uint32_t sweep0, uint32_t fuse, void *stream);
/* Action::heatbath_update / overrelaxation_update(state, l) on a 2-D action (gffaction.cc:33-42,68-77;
 * quenchedschwingeraction.cc:46-65; nonlinearsigmaaction.cc:24-91): as mlmcpi_path_site_updates; l is a vertex (GFF, sigma
 * model: both angles of the vertex) or link (Schwinger) index. */
int mlmcpi_lattice_site_updates(const mlmcpi_lattice_action *act, double *d_state, uint32_t B, const uint32_t *d_sites,
                                uint32_t n, uint32_t site, int32_t heat, uint64_t seed, uint32_t chain0, uint32_t step,
                                void *stream);
/* OverrelaxedHeatBathSampler::draw with random_order = true (sampler/overrelaxedheatbathsampler.cc:8-31: the index set is
 * shuffled before every sweep, then one local update per index), parallel within a chain: GFF, Schwinger and the sigma model.
 * ORDER: index l of a chain (Schwinger: the 2 Mt Mx links; GFF, sigma model: the Mt Mx vertices -- the index set
 * mlmcpi_lattice_site_updates walks) takes word l & 3 of Philox (site l >> 2, chain0 + b, step sweep0 + s, purpose 18, sub 0) as
 * its 32-bit key; sweep s visits the indices in ascending (key, l).  Every chain and every sweep has its own order; results do
 * not depend on the batch split.  The updates run in rounds (round of an index = 1 + the largest round of the indices it
 * shares a stencil with that precede it), one workgroup per chain, all n_overrelax + n_heatbath sweeps in ONE launch, and give
 * exactly what mlmcpi_lattice_site_updates gives when it walks that order: same arithmetic, same random numbers (step
 * sweep0 + s).  Mt, Mx >= 2, odd extents included.  The state lives in LDS where it fits (Schwinger 64 x 64, GFF 96 x 96,
 * sigma model 64 x 64), in global memory beyond (any lattice; MLMCPI_RANDOM_SWEEP_HOME=global through mlmcpi_set_option forces
 * it; MLMCPI_RANDOM_SWEEP_CHUNK=k, 1 <= k <= 254, sets how many rounds are scheduled at a time: neither changes a bit).
 *   d_work   workspace of mlmcpi_lattice_random_sweep_workspace_bytes() bytes (keys, rounds: no need to zero it)
 * Other kinds: MLMCPI_ERR_UNSUPPORTED (the 1-D paths keep mlmcpi_path_site_updates). */
int mlmcpi_lattice_random_sweep_workspace_bytes(const mlmcpi_lattice_action *act, uint32_t B, size_t *bytes);
int mlmcpi_lattice_random_sweep_draw(const mlmcpi_lattice_action *act, double *d_state, uint32_t B, uint32_t n_overrelax,
                                     uint32_t n_heatbath, uint64_t seed, uint32_t chain0, uint32_t sweep0, void *d_work, void *stream);
/* The order and the schedule of sweep `sweep` of mlmcpi_lattice_random_sweep_draw (the shuffle of
 * sampler/overrelaxedheatbathsampler.cc:8-31), so that a caller can walk the very same order through
 * mlmcpi_lattice_site_updates: d_order [B][n] the indices in visiting order, d_round [B][n] (may be NULL) the round of each
 * index, counted from 1.  Synchronises nothing; uses the library's scratch buffer of the stream. */
int mlmcpi_lattice_random_sweep_order(const mlmcpi_lattice_action *act, uint32_t B, uint64_t seed, uint32_t chain0, uint32_t sweep,
                                      uint32_t *d_order /* [B][n] indices in visiting order */,
                                      uint32_t *d_round /* [B][n] round of each index, may be NULL */, void *stream);
/* Same, without the final device-to-device copy: the sweeps ping-pong between d_a (input) and d_b;
 * *result_in_b tells the caller which buffer holds the result (swap your pointers when it is 1). */
int mlmcpi_lattice_sweep_draw_pingpong(const mlmcpi_lattice_action *act, double *d_a, double *d_b, uint32_t B,
                                       uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0,
                                       uint32_t sweep0, uint32_t fuse, int32_t *result_in_b, void *stream);
/* Same, with the input left untouched: the first launch reads d_src (never written), the launches then alternate between
 * the work buffers d_w0 and d_w1; *result_in = 0 / 1 names the work buffer that holds the result.  d_w1 may equal
 * d_src (then this is the ping-pong form).  This is what Sampler::draw(out) needs to hand `out` the new sample without a
 * copy while the caller still holds the previous one (sampler/overrelaxedheatbathsampler.cc:30 copies the state out). */
int mlmcpi_lattice_sweep_draw_from(const mlmcpi_lattice_action *act, const double *d_src, double *d_w0, double *d_w1,
                                   uint32_t B, uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0,
                                   uint32_t sweep0, uint32_t fuse, int32_t *result_in, void *stream);
/* mlmcpi_lattice_sweep_draw_from with the QoI of the new sample summed inside the draw's last launch, while the tile is
 * still in LDS: Sampler::draw + QoI::evaluate of the loop at montecarlo/montecarlosinglelevel.cc:59-77 in one pass over
 * the state instead of two.  qoi_kind 1 = QoIAvgPlaquette (qoi/qft/qoiavgplaquette.cc:8-27), 2 = QoI2DSusceptibility
 * (qoi/qft/qoi2dsusceptibility.cc:8-27), both for the quenched Schwinger action; 3 = QoI2DPhiSquared
 * (qoi/qft/qoi2dphisquared.cc:8-15) for the GFF action; 4 = QoI2DMagneticSusceptibility
 * (qoi/qft/qoi2dmagneticsusceptibility.cc:7-21) for the sigma model; d_qoi[b].  n_heatbath >= 1 (the draw has to end with a heat-bath
 * sweep) and a QoI of the action at hand: MLMCPI_ERR_UNSUPPORTED otherwise, and the caller evaluates the QoI
 * separately.  Same values as mlmcpi_qoi_* on the result up to the order of the summation. */
int mlmcpi_lattice_sweep_draw_qoi(const mlmcpi_lattice_action *act, const double *d_src, double *d_w0, double *d_w1, uint32_t B,
                                  uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0, uint32_t sweep0,
                                  uint32_t fuse, int32_t qoi_kind, double *d_qoi, int32_t *result_in, void *stream);
/* One pass of the sampling loop at montecarlo/montecarlosinglelevel.cc:59-77 in one call: sampler->draw, qoi->evaluate and
 * stats->record_sample -- mlmcpi_lattice_sweep_draw_qoi followed by mlmcpi_stats_accumulate(d_acc, d_qoi, B), with the
 * moments updated by the launch that finishes the QoI (one launch less per sample; same values).  d_acc[B][5] as for
 * mlmcpi_stats_accumulate. */
int mlmcpi_lattice_sweep_draw_qoi_record(const mlmcpi_lattice_action *act, const double *d_src, double *d_w0, double *d_w1,
                                         uint32_t B, uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0,
                                         uint32_t sweep0, uint32_t fuse, int32_t qoi_kind, double *d_qoi, double *d_acc,
                                         int32_t *result_in, void *stream);
/* The launch plan of a draw: the launches mlmcpi_lattice_sweep_draw* issues for (act, B, n_overrelax, n_heatbath, fuse) under
 * the options in force (mlmcpi_set_option), in order -- from the very planner the draws run, without touching a device.
 * Kernels (namespace mlmcpi) and the template arguments a record fixes: */
enum mlmcpi_sweep_kernel {
  MLMCPI_K_SCHWINGER_SWEEP = 0,     /* schwinger_sweep_kernel<n_heatbath != 0, threads, TWC, THC, step>; TWC x THC = tile_w x tile_h
                                     * with fixed_tile, else 0 x 0 */
  MLMCPI_K_GFF_SWEEP = 1,           /* gff_sweep_kernel<n_heatbath != 0, threads, TWC, THC> */
  MLMCPI_K_SCHWINGER_OR_BLOCK = 2,  /* schwinger_or_block_kernel<n_overrelax> */
  MLMCPI_K_GFF_OR_BLOCK = 3,        /* gff_or_block_kernel<n_overrelax, tile_w> */
  MLMCPI_K_GFF_OR_HEAT = 4,         /* gff_or_heat_kernel<n_overrelax, tile_w> */
  MLMCPI_K_SCHWINGER_PERM = 5,      /* schwinger_perm_kernel<tile_h> */
  MLMCPI_K_SCHWINGER_PERM_HEAT = 6, /* schwinger_perm_heat_kernel<threads, step> */
  MLMCPI_K_SIGMA_SWEEP = 7          /* sigma_sweep_kernel<threads> */
};
typedef struct mlmcpi_sweep_launch {
  uint32_t kernel;                  /* enum mlmcpi_sweep_kernel */
  uint32_t n_overrelax, n_heatbath; /* the sweeps the launch covers, overrelaxation first (the depth K of the fused kernels) */
  uint32_t grid_x, threads;         /* workgroups per chain (grid.y = B) and threads per workgroup */
  uint32_t lds_bytes;               /* dynamic LDS */
  uint32_t tile_w, tile_h, tiles_x; /* owned tile and tiles per row of tiles */
  uint32_t fixed_tile;              /* 1: the tile extents are template arguments of the generic kernels */
  uint32_t step;                    /* 1: Schwinger heat bath from the step envelope (2 beta <= 16), 0: wrapped Cauchy */
  uint32_t planes;                  /* closed-form kernels: builds of the plane of plaquettes per workgroup, 1 since the plane is packed to its read set (else 0) */
  uint32_t pool_cap;                /* schwinger_sweep_kernel heat bath: entries of the list of open cells */
  uint32_t kinds;                   /* generic kernels: bit q set = sweep q of the launch is a heat-bath sweep */
} mlmcpi_sweep_launch;
/* Same argument checks as the draws (even extents, square GFF lattice, B > 0).  Writes min(*count, capacity) records to `out`
 * and the number of launches to *count; MLMCPI_ERR_INVALID, with *count set, when capacity is too small (call with
 * capacity 0 to ask).  Record this beside a checkpoint: see BIT REPRODUCIBILITY ACROSS LAUNCH PLANS above. */
int mlmcpi_lattice_sweep_plan(const mlmcpi_lattice_action *act, uint32_t B, uint32_t n_overrelax, uint32_t n_heatbath,
                              uint32_t fuse, mlmcpi_sweep_launch *out, uint32_t capacity, uint32_t *count);
/* Action::copy_from_fine / copy_from_coarse between a lattice and its next-coarser level, coarsening
 * factors rt, rx in {1, 2} in the temporal / spatial direction (CoarsenBoth = 2,2; CoarsenTemporal = 2,1;
 * CoarsenSpatial = 1,2; lattice/lattice2d.cc:24-47).  `fine` describes the FINE lattice.
 *   Schwinger (quenchedschwingeraction.cc:92-195): coarse links = mod_2pi(sum of the fine links they span);
 *     copy_from_coarse halves a coarse link over its two fine links and leaves the fine-only links untouched.
 *   GFF (gffaction.cc:97-118): vertices (rt i, rx j) <-> (i, j). */
int mlmcpi_lattice_copy_from_fine(const mlmcpi_lattice_action *fine, uint32_t rt, uint32_t rx, const double *d_fine,
                                  double *d_coarse, uint32_t B, void *stream);
int mlmcpi_lattice_copy_from_coarse(const mlmcpi_lattice_action *fine, uint32_t rt, uint32_t rx, const double *d_coarse,
                                    double *d_fine, uint32_t B, void *stream);
/* TwoLevelMetropolisStep::draw (montecarlo/twolevelmetropolisstep.cc:35-89) on the quenched Schwinger lattice:
 * copy_from_coarse, the conditioned fine action's fill_fine_points and evaluate, copy_from_fine, the three action
 * differences, the Metropolis test and the copy of accepted states.  Conditioned fine action by coarsening
 * (quenchedschwingerconditionedfineaction.hh:218-238):
 *   one direction halved (CoarsenTemporal / CoarsenSpatial / levels of CoarsenAlternate):
 *     QuenchedSchwingerSemiConditionedFineAction (.cc:130-204, 332-379): uniform shifts + ExpCos draws;
 *   both directions halved (CoarsenBoth): QuenchedSchwingerConditionedFineAction (.cc:7-78, 207-289):
 *     BesselProductDistribution for beta <= 8, ApproximateBesselProductDistribution beyond.
 * `coarse` carries the coarse lattice extents and the coarse beta (QuenchedSchwingerAction::coarse_action).
 *   d_phi_coarse [B][2 Mt_c Mx_c]  coarse-level proposal;  d_theta [B][2 Mt Mx]  current fine state (updated when
 *   accepted);  d_accept [B];  d_terms [B][3] = (dS_fine, dS_coarse, dS_trial) or NULL. */
int mlmcpi_lattice_twolevel_workspace_bytes(const mlmcpi_lattice_action *fine, const mlmcpi_lattice_action *coarse,
                                            uint32_t B, size_t *bytes);
int mlmcpi_lattice_twolevel_draw(const mlmcpi_lattice_action *fine, const mlmcpi_lattice_action *coarse,
                                 const double *d_phi_coarse, double *d_theta, uint32_t B, uint64_t seed,
                                 uint32_t chain0, uint32_t step, void *d_work, int32_t *d_accept, double *d_terms,
                                 void *stream);
/* The same step with the conditioned fine action chosen by the caller: cfa_kind 0 = what the reference's factory picks
 * for the lattice (quenchedschwingerconditionedfineaction.hh:218-238), 1 = QuenchedSchwingerGaussianConditionedFineAction
 * (quenchedschwingerconditionedfineaction.cc:81-134, 293-327; lattices coarsened in both directions): uniform splits of
 * the coarse links, the four interior links of every 2 x 2 block from GaussianFillinDistribution
 * (distribution/gaussianfillindistribution.{hh,cc}; Philox purpose 13 of the coarse cell). */
int mlmcpi_lattice_twolevel_draw_cfa(const mlmcpi_lattice_action *fine, const mlmcpi_lattice_action *coarse, int32_t cfa_kind,
                                     const double *d_phi_coarse, double *d_theta, uint32_t B, uint64_t seed, uint32_t chain0,
                                     uint32_t step, void *d_work, int32_t *d_accept, double *d_terms, void *stream);
/* Exact sampler of the Gaussian free field: GFFAction::draw / initialise_state (action/qft/gffaction.cc:121-123,
 * 200-213; the reference goes through a sparse Cholesky factor built by Eigen, which it cannot build beyond ~64^2).
 * On the periodic lattice the precision matrix is diagonal in Fourier space, so the draw is a spectral synthesis:
 *   phi(x) = Re sum_k (n0_k + i n1_k) e^{+i k x} / sqrt(N lambda(k)),  lambda(k) = 4 + mu2 - 2 cos(2 pi k_t/Mt) - 2 cos(2 pi k_x/Mx),
 * normals of mode l = k_x Mt + k_t from Philox (site l, purpose P_EXACT, step `step`); batched 2-D inverse FFT (hipFFT).
 * d_work: mlmcpi_lattice_exact_workspace_bytes (one complex field per chain). */
int mlmcpi_lattice_exact_workspace_bytes(const mlmcpi_lattice_action *act, uint32_t B, size_t *bytes);
int mlmcpi_lattice_exact_draw(const mlmcpi_lattice_action *act, double *d_phi, uint32_t B, uint64_t seed, uint32_t chain0,
                              uint32_t step, void *d_work, void *stream);
/* ---- Gaussian free field: levels of a coarsening hierarchy and the two-level step between them ------
 * A level = GFFAction(lattice, fine_lattice, mass, n_gibbs_smooth, omega) (action/qft/gffaction.hh:120-146) on the lattice
 * (Mt, Mx, coarsening type, coarsening level); CoarsenRotate levels of odd depth are rotated lattices
 * (lattice/lattice2d.hh:98-437).  The reference's coarse_action() is (coarse lattice, mass, n_gibbs_smooth = 2, omega = 1)
 * (gffaction.hh:201-208).  Levels with n_gibbs_smooth > 0 evaluate 1/2 phi^T Qhat phi with the dense smoothed precision
 * matrix of gffaction.cc:126-173 (built on the host, levels of up to 4096 vertices); index maps come from tables like the
 * reference's.  The finest level of a run keeps using mlmcpi_lattice_* (stencil kernels, FFT sampler). */
typedef struct mlmcpi_gff_level mlmcpi_gff_level;
int mlmcpi_gff_level_create(uint32_t Mt, uint32_t Mx, int32_t coarsening_type, int32_t level, double mass, int32_t n_gibbs_smooth,
                            double omega, mlmcpi_gff_level **out);
int mlmcpi_gff_level_destroy(mlmcpi_gff_level *level);
/* sample_size; number of vertices / extents of the next-coarser lattice (0 if there is none); mu2 (gffaction.hh:174-181) */
int mlmcpi_gff_level_info(const mlmcpi_gff_level *level, uint32_t *n_vertices, uint32_t *n_coarse, uint32_t *Mt_coarse,
                          uint32_t *Mx_coarse, double *mu2);
/* lattice2d.cc:82-134 (host): pairs[2 n_coarse] = (fine index, coarse index) ascending in the fine index = fine2coarse_map;
 * fineonly[n_vertices - n_coarse] ascending = fineonly_vertices */
int mlmcpi_gff_level_tables(const mlmcpi_gff_level *level, uint32_t *pairs, uint32_t *fineonly);
/* host copies of the dense matrices, row major [N][N]: which = 0 Qhat (gffaction.cc:165-167), 1 inverse of the Cholesky
 * factor of the plain precision matrix (the exact sampler, gffaction.cc:169-173) */
int mlmcpi_gff_level_matrix(mlmcpi_gff_level *level, int32_t which, double *h_out);
/* GFFAction::evaluate (gffaction.cc:8-30) */
int mlmcpi_gff_level_evaluate(mlmcpi_gff_level *level, const double *d_phi, uint32_t B, double *d_S, void *stream);
/* GFFAction::draw (gffaction.cc:200-213): exact draw + n_gibbs_smooth lexicographic sweeps of
 * global_heatbath_update_eff (:45-66); Philox (pair l >> 1, branch l & 1) with purpose 12 (white noise) / 11 (sweep k = sub) */
int mlmcpi_gff_level_draw(mlmcpi_gff_level *level, double *d_phi, uint32_t B, uint64_t seed, uint32_t chain0, uint32_t step,
                          void *stream);
/* GFFAction::copy_from_fine / copy_from_coarse (gffaction.cc:97-118); `fine` is the finer of the two levels */
int mlmcpi_gff_copy_from_fine(mlmcpi_gff_level *fine, const double *d_fine, double *d_coarse, uint32_t B, void *stream);
int mlmcpi_gff_copy_from_coarse(mlmcpi_gff_level *fine, const double *d_coarse, double *d_fine, uint32_t B, void *stream);
/* GFFConditionedFineAction (gffconditionedfineaction.cc:7-49): fill_fine_points (fine-only vertex l ~ N(sigma^2 Delta,
 * sigma^2), normal = Philox(site l, purpose 7); d_S[b] = the conditioned action of the filled state) and evaluate */
int mlmcpi_gff_cfa_fill(mlmcpi_gff_level *fine, double *d_state, uint32_t B, uint64_t seed, uint32_t chain0, uint32_t step,
                        double *d_S, void *stream);
int mlmcpi_gff_cfa_evaluate(mlmcpi_gff_level *fine, const double *d_state, uint32_t B, double *d_S, void *stream);
/* TwoLevelMetropolisStep::draw (twolevelmetropolisstep.cc:35-89) for a GFF level and its coarsening: d_theta is the current
 * fine state (updated in place on acceptance), d_terms[b] = (dS_fine, dS_coarse, dS_trial) (may be NULL) */
int mlmcpi_gff_twolevel_workspace_bytes(const mlmcpi_gff_level *fine, uint32_t B, size_t *bytes);
int mlmcpi_gff_twolevel_draw(mlmcpi_gff_level *fine, mlmcpi_gff_level *coarse, const double *d_phi_coarse, double *d_theta,
                             uint32_t B, uint64_t seed, uint32_t chain0, uint32_t step, void *d_work, int32_t *d_accept,
                             double *d_terms, void *stream);

/* ---- O(3) nonlinear sigma model: levels of the CoarsenRotate hierarchy and the two-level step ---------
 * A level by value: (Mt, Mx) are the extents of the Cartesian frame of Lattice2D, both even and >= 2 (Mt Mx <= 2^30);
 * rotated = 0: the Mt Mx vertices of mlmcpi_lattice_action, l = Mt j + i; rotated != 0: the Mt Mx / 2 vertices with (i + j)
 * even in the reference's order (lattice2d.hh:230-268), two planes of Mt/2 x Mx/2, the even-even plane E then the odd-odd plane
 * O, index p (Mt Mx / 4) + (Mt/2) b + a = vertex (2 a + p, 2 b + p).  State [B][2 n]: (theta, phi) of vertex l at 2 l, 2 l + 1.
 * Rotated neighbours in the reference's order (+1,+1), (+1,-1), (-1,+1), (-1,-1): E(a, b): O(a, b), O(a, b-1), O(a-1, b),
 * O(a-1, b-1); O(a, b): E(a+1, b+1), E(a+1, b), E(a, b+1), E(a, b) (periodic).  The coarse partner of the unrotated (Mt, Mx)
 * is the rotated (Mt, Mx); that of the rotated (Mt, Mx) is the unrotated (Mt/2, Mx/2) (lattice2d.cc:83-108). */
typedef struct mlmcpi_sigma_level {
  uint32_t Mt, Mx;
  int32_t rotated;
  double beta;
} mlmcpi_sigma_level;
/* _state_size: 2 n.  _initialise: the map of mlmcpi_lattice_initialise over the level's 2 n entries.  _evaluate: S = -1/2 beta
 * sum_n sigma_n . Delta_n; rotated: as the bond sum -beta sum_E sigma_E . Delta_E; unrotated: mlmcpi_lattice_evaluate.
 * _magnetic_susceptibility: |sum_n sigma_n|^2 / n with the level's n.
 * _sweep_draw: OverrelaxedHeatBathSampler::draw on the level, d_state in place, d_scratch of the same size; unrotated:
 * mlmcpi_lattice_sweep_draw (fuse 0).  Rotated: a sweep is phase E then phase O; heat bath of vertex l in sweep s = ONE Philox
 * call (site l = the level's vertex index, chain, step sweep0 + s, purpose 14); the canonical form of the unrotated kernel, so a
 * draw is bit-identical whatever MLMCPI_SIGMA_LEVEL_PLAN=TWxTHxNTxK (mlmcpi_set_option: tile of plane cells, TW, TH in 1..128,
 * workgroup NT in {256, 512, 1024}, K in 1..16 sweeps fused per launch, within the LDS) and whatever the batch split.
 * _copy_from_fine / _copy_from_coarse (NonlinearSigmaAction::copy_from_*, nonlinearsigmaaction.cc:113-139): `fine` is the FINE
 * level, the other state lives on its coarse partner; _copy_from_coarse leaves the fine-only entries untouched. */
int mlmcpi_sigma_level_state_size(const mlmcpi_sigma_level *level, uint32_t *n);
int mlmcpi_sigma_level_initialise(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint64_t seed, uint32_t chain0,
                                  void *stream);
int mlmcpi_sigma_level_evaluate(const mlmcpi_sigma_level *level, const double *d_state, uint32_t B, double *d_S, void *stream);
int mlmcpi_sigma_level_magnetic_susceptibility(const mlmcpi_sigma_level *level, const double *d_state, uint32_t B, double *d_out,
                                               void *stream);
int mlmcpi_sigma_level_sweep_draw(const mlmcpi_sigma_level *level, double *d_state, double *d_scratch, uint32_t B,
                                  uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0, uint32_t sweep0,
                                  void *stream);
int mlmcpi_sigma_level_copy_from_fine(const mlmcpi_sigma_level *fine, const double *d_fine, double *d_coarse, uint32_t B,
                                      void *stream);
int mlmcpi_sigma_level_copy_from_coarse(const mlmcpi_sigma_level *fine, const double *d_coarse, double *d_fine, uint32_t B,
                                        void *stream);
/* The zero-momentum (time-slice) two-point function on a level (sigma_correlator.hip); rotated = 0 is the plain
 * lattice.  Vertices (i, j), 0 <= i < Mt, 0 <= j < Mx (a rotated level holds those with i + j even), N = the level's n.
 *   slice sums   S^t_i = sum_j sigma(i, j) over the level's vertices with first coordinate i;  S^x_j = sum_i sigma(i, j).  On a
 *                rotated level a slice holds Mx/2 (Mt/2) vertices and all Mt (Mx) slices exist.
 *   correlators  C_t(tau) = (1/N) sum_i S^t_i . S^t_{(i + tau) mod Mt}, tau = 0 .. Mt/2;
 *                C_x(tau) = (1/N) sum_j S^x_j . S^x_{(j + tau) mod Mx}, tau = 0 .. Mx/2.
 * d_out [B][n_out], n_out = (Mt/2 + 1) + (Mx/2 + 1) (_correlator_size), C_t first.  With w(0) = w(M/2) = 1 and w = 2 otherwise (an
 * extent of 2: tau = 0, 1, both weight 1), sum_tau w C_d = chi_m = |sum sigma|^2 / N in both directions, and F_d = sum_tau w C_d
 * cos(2 pi tau / M_d) = |sum_i S_i exp(2 pi i i / M_d)|^2 / N is the structure factor at the lowest momentum; the second-moment
 * correlation length xi_2,d = sqrt(chi_m / F_d - 1) / (2 sin(pi / M_d)) is host arithmetic on means (include/mlmcpi/qoi.hh).
 * d_acc (may be NULL) [B][n_out][2]: C is ADDED to [.][.][0] and C^2 to [.][.][1] in the launch that writes d_out; the caller
 * counts the calls.  d_work: _correlator_workspace_bytes(level, B) bytes, 256-byte aligned; content at entry ignored.  The state
 * is read once (one sincos pair per vertex); every sum is taken in an order fixed by the level alone, without atomics, so a
 * chain's output is the same bits whatever B and however the chains are split over calls.  The launch geometry takes B <= 65535
 * chains per call (CHAINS PER CALL above).  MLMCPI_ERR_INVALID, with nothing launched: NULL level, odd or zero extents, Mt Mx > 2^30, NULL d_state, d_out
 * or d_work, B = 0 or B > 65535, work_bytes below _correlator_workspace_bytes. */
int mlmcpi_sigma_level_correlator_size(const mlmcpi_sigma_level *level, uint32_t *n_out);
int mlmcpi_sigma_level_correlator_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes);
int mlmcpi_sigma_level_correlator(const mlmcpi_sigma_level *level, const double *d_state, uint32_t B, double *d_out,
                                  double *d_acc /* may be NULL */, void *d_work, size_t work_bytes, void *stream);
/* The geometric (Berg-Luescher) topological charge on a level and its susceptibility (sigma_topology.hip);
 * rotated = 0 is the plain lattice, `beta` is ignored.  With sigma = (sin theta cos phi, sin theta sin phi, cos theta) and, for an
 * ordered triple of unit vectors, A(a, b, c) = 2 atan2(a . (b x c), 1 + a . b + b . c + c . a):
 *   plain level    one face per vertex (i, j): corners s1 = (i, j), s2 = (i+1, j), s3 = (i+1, j+1), s4 = (i, j+1), periodic;
 *                  triangles (s1, s2, s3) and (s1, s3, s4)
 *   rotated level  one face per site (i, j) with i + j odd (n faces for n vertices): corners W = (i-1, j), S = (i, j-1),
 *                  E = (i+1, j), N = (i, j+1), all level vertices, periodic in the Cartesian frame; triangles (W, S, E), (W, E, N)
 *   Q = (1 / 4 pi) sum over faces (A_1 + A_2), not rounded;  chi = Q^2 / n with the level's n.
 * d_q [n_chains] and d_chi [n_chains]: either may be NULL, not both.  d_acc (may be NULL) [n_chains][5]: stats->record_sample of
 * chi in the launch that finishes it (mlmcpi_stats_accumulate's recurrence).  The state is read once (one sincos pair per vertex,
 * staged in LDS tile by tile with the halo the tile's faces reach); lane, wave and tile partials are added in an order fixed by
 * the level alone, without atomics; the partials live in the library's scratch.  A chain's outputs are the same bits for every
 * n_chains, every split of the chains over calls, every stream and whichever outputs are asked for.  Any n_chains runs (CHAINS
 * PER CALL above).  MLMCPI_ERR_INVALID, with nothing launched: NULL level or d_state, d_q and d_chi both NULL, odd or zero
 * extents, Mt Mx > 2^30, n_chains = 0. */
int mlmcpi_sigma_level_topological_charge(const mlmcpi_sigma_level *level, const double *d_state, uint32_t n_chains,
                                          double *d_q /* may be NULL */, double *d_chi /* may be NULL */,
                                          double *d_acc /* may be NULL: record_sample moments of chi, [n_chains][5] */, void *stream);
/* Cooling on a level and the cooled charge (sigma_cooling.hip, a smoother of sigma_smooth.hip on the field of sigma_field.hip;
 * DESIGN.md 4.1g); `beta` is ignored.  Cooling is the deterministic
 * beta -> infinity limit of the heat bath: sigma_l <- Delta_l / |Delta_l|, Delta_l = add4 of the four neighbours in the order of
 * mlmcpi_sigma_level_sweep_draw, |Delta| = sqrt((x^2 + y^2) + z^2), three divisions; Delta_l = 0 leaves sigma_l as it is.  One
 * cooling sweep updates the two colour classes in the sweeps' order: plain level (i + j) even, then odd; rotated level phase E,
 * then phase O.  Depth d is the field after d sweeps, starting from sigma_of(d_state); between sweeps the field lives as unit
 * vectors and is never converted back to angles.  For every depth d = depths[k]:
 *   d_q      [n_chains][n_depths]  Q_d, the charge above on the field of depth d (same faces, triangles and sum order)
 *   d_chi    [n_chains][n_depths]  Q_d^2 / n
 *   d_energy [n_chains][n_depths]  E_d = 2 n - (1/2) sum_l sigma_l . Delta_l, the bond energy sum_bonds (1 - sigma . sigma'),
 *                                  coinciding neighbours of tiny levels counted as often as they occur
 * any of the three may be NULL, not all.  d_cooled (may be NULL) [n_chains][2 n]: the angles (atan2(sqrt(x^2 + y^2), z),
 * atan2(y, x)) of the field at the LAST depth.  depths (HOST memory) is strictly ascending, may start at 0, 1 <= n_depths <=
 * MLMCPI_SIGMA_COOLING_MAX_DEPTHS, last depth <= MLMCPI_SIGMA_COOLING_MAX_DEPTH.  d_state is read once and never written.
 * d_work: _cooling_workspace_bytes(level, n_chains) bytes, 256-byte aligned, content at entry ignored: two buffers of unit
 * vectors ([n_chains][3][n] doubles each, ping-pong) and the partial sums of the charge (one per 32 x 32 tile) and of the energy
 * (one per group of 256 vertices).  The library does not chunk: a caller short of memory splits the chains.
 * An update is a function of four stored vectors and every sum is taken in an order fixed by the level alone, without atomics: a
 * chain's Q_d, chi_d, E_d and cooled state are the same bits under every MLMCPI_SIGMA_COOL_PLAN=TWxTHxNTxK (tile, workgroup size,
 * sweeps fused per launch; a launch never runs past the next listed depth), every n_chains, split of the chains over calls and
 * stream, every choice of outputs and EVERY DEPTH LIST CONTAINING d; Q_0 and chi_0 are the bits of
 * mlmcpi_sigma_level_topological_charge.  Any n_chains runs (CHAINS PER CALL above).  MLMCPI_ERR_INVALID, with nothing launched:
 * NULL level, d_state, depths or d_work; d_q, d_chi and d_energy all NULL; odd or zero extents, Mt Mx > 2^30; n_chains = 0;
 * n_depths outside 1 .. 32; depths not strictly ascending or beyond 4096; work_bytes below the query; more workgroups in a launch
 * than the grid holds.
 * _cooling_plan (host only, touches no device) reports the launches of such a call and returns the status the call would for the
 * arguments it sees. */
#define MLMCPI_SIGMA_COOLING_MAX_DEPTHS 32
#define MLMCPI_SIGMA_COOLING_MAX_DEPTH 4096
typedef struct mlmcpi_sigma_cooling_plan {
  uint32_t tw, th, nt, fuse;  /* tile (plain: vertices, rotated: plane cells; never larger than the plane), workgroup size, sweeps per launch at most */
  uint32_t tiles;             /* cooling workgroups per chain and launch */
  uint32_t lds_bytes;         /* LDS image of the deepest launch */
  uint32_t n_launches;        /* cooling launches of the call */
  uint32_t n_measurements;    /* = n_depths */
  uint8_t launch_sweeps[MLMCPI_SIGMA_COOLING_MAX_DEPTH]; /* [n_launches] sweeps of each; they sum to the last depth, none crosses a listed depth */
} mlmcpi_sigma_cooling_plan;
int mlmcpi_sigma_level_cooling_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t n_chains, size_t *bytes);
int mlmcpi_sigma_level_cooled_charge(const mlmcpi_sigma_level *level, const double *d_state, uint32_t n_chains,
                                     const uint32_t *depths /* host */, uint32_t n_depths, double *d_q /* may be NULL */,
                                     double *d_chi /* may be NULL */, double *d_energy /* may be NULL */,
                                     double *d_cooled /* may be NULL */, void *d_work, size_t work_bytes, void *stream);
int mlmcpi_sigma_level_cooling_plan(const mlmcpi_sigma_level *level, uint32_t n_chains, const uint32_t *depths, uint32_t n_depths,
                                    mlmcpi_sigma_cooling_plan *plan);
/* Gradient flow on a level and the flowed charge (sigma_flow.hip, the other smoother of sigma_smooth.hip); `beta`
 * is ignored.  With F(Y)_l = Delta_l -
 * (Y_l . Delta_l) Y_l, Delta_l = add4 of the four neighbours' Y in the order of mlmcpi_sigma_level_sweep_draw and the dot product
 * (x x' + y y') + z z', one step of size eps is the 2N-storage third-order Runge-Kutta scheme, on ALL sites from the previous
 * stage's Y, starting from A = 0, Y = sigma:  A <- a_i A + eps F(Y), Y <- Y + b_i A, i = 1, 2, 3, a = (0, -17/32, -32/27), b =
 * (1/4, 8/9, 3/4); then sigma <- Y / |Y|, |Y| = sqrt((x^2 + y^2) + z^2), three divisions.  Stage values are not normalised.
 * Step count s is the field after s steps, flow time t = s eps, starting from sigma_of(d_state); between steps the field lives
 * as unit vectors and is never converted back to angles.  For every s = steps[k], d_q, d_chi and d_energy [n_chains][n_steps]
 * are Q_s, Q_s^2 / n and E_s as in mlmcpi_sigma_level_cooled_charge (any may be NULL, not all); d_flowed (may be NULL)
 * [n_chains][2 n]: the angles of the field at the LAST step count.  steps (HOST memory) is strictly ascending, may start at 0,
 * 1 <= n_steps <= MLMCPI_SIGMA_FLOW_MAX_TIMES, last entry <= MLMCPI_SIGMA_FLOW_MAX_STEPS; eps is finite, 0 < eps <= 0.25 (the
 * energy never rose for eps <= 0.3 and blew up at 0.4).  d_state is read once and never written.  d_work:
 * _flow_workspace_bytes(level, n_chains) bytes, 256-byte aligned, content at entry ignored, the layout of cooling's workspace.
 * A stage update is a function of the stored Y and A of the site and the stored Y of four neighbours, and every sum is taken in
 * an order fixed by the level alone, without atomics: a chain's Q_s, chi_s, E_s and flowed state are the same bits under every
 * MLMCPI_SIGMA_FLOW_PLAN=TWxTHxNTxK (tile, workgroup size, steps fused per launch; a launch never runs past the next listed step
 * count), every n_chains, split of the chains over calls and stream, every choice of outputs and EVERY STEP LIST CONTAINING s;
 * Q_0 and chi_0 are the bits of mlmcpi_sigma_level_topological_charge.  Any n_chains runs (CHAINS PER CALL above).
 * MLMCPI_ERR_INVALID, with nothing launched: NULL level, d_state, steps or d_work; d_q, d_chi and d_energy all NULL; odd or zero
 * extents, Mt Mx > 2^30; n_chains = 0; eps outside (0, 0.25] or not finite; n_steps outside 1 .. 32; steps not strictly
 * ascending or beyond 4096; work_bytes below the query; more workgroups in a launch than the grid holds.
 * _flow_plan (host only, touches no device) reports the launches of such a call and returns the status the call would for the
 * arguments it sees. */
#define MLMCPI_SIGMA_FLOW_MAX_TIMES 32
#define MLMCPI_SIGMA_FLOW_MAX_STEPS 4096
typedef struct mlmcpi_sigma_flow_plan {
  uint32_t tw, th, nt, fuse;  /* tile (plain: vertices, rotated: plane cells; never larger than the plane), workgroup size, steps per launch at most */
  uint32_t tiles;             /* flow workgroups per chain and launch */
  uint32_t lds_bytes;         /* LDS image of the deepest launch: (tw + 6 K)(th + 6 K) x 72 B (rotated: 144 B) */
  uint32_t n_launches;        /* flow launches of the call */
  uint32_t n_measurements;    /* = n_steps */
  uint8_t launch_steps[MLMCPI_SIGMA_FLOW_MAX_STEPS]; /* [n_launches] steps of each; they sum to the last step count, none crosses a listed one */
} mlmcpi_sigma_flow_plan;
int mlmcpi_sigma_level_flow_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t n_chains, size_t *bytes);
int mlmcpi_sigma_level_flowed_charge(const mlmcpi_sigma_level *level, const double *d_state, uint32_t n_chains, double eps,
                                     const uint32_t *steps /* host */, uint32_t n_steps, double *d_q /* may be NULL */,
                                     double *d_chi /* may be NULL */, double *d_energy /* may be NULL */,
                                     double *d_flowed /* may be NULL */, void *d_work, size_t work_bytes, void *stream);
int mlmcpi_sigma_level_flow_plan(const mlmcpi_sigma_level *level, uint32_t n_chains, double eps, const uint32_t *steps,
                                 uint32_t n_steps, mlmcpi_sigma_flow_plan *plan);
/* The Wolff single-cluster update on a level (sigma_cluster.hip): n_updates updates of every chain of
 * d_state [B][2 n], in place.  Unrotated: mlmcpi_sigma_cluster_* on (Mt, Mx, beta), the same bits.  Rotated: the level is
 * bipartite, every link has one E end; its 2 n links are (e, d), e an E vertex (e < n / 2), d its direction in the order above;
 * from O(a, b), direction d' crosses link (neighbour, 3 - d').  Where a plane extent is 1 several neighbours of a vertex
 * coincide: distinct links, a uniform each.  Philox, step = update0 + k: purpose 19 site 0 sub 0 (u, v) -> r (r_z = 1 - 2 u,
 * azimuth 2 pi v - pi), sub 1 u -> seed vertex min(floor(u n), n - 1); purpose 20 site e sub d >> 1: u decides link (e, d) for
 * d even, v for d odd.  With a_l = r . sigma_l BEFORE the update, link (x, y) is bonded iff (a_x a_y) > 0 and its uniform <
 * 1 - exp(min(0, -2 beta (a_x a_y))); the component of the seed is reflected, sigma' = sigma - 2 a r, canonical form.  The
 * state does not depend on launch plan (MLMCPI_SIGMA_CLUSTER_TEAM / _BITMAP govern this kernel too), batch split, chain0
 * or call split.  Workspace: 12 B per vertex and chain (the queue) plus a bit per vertex; its content at entry is ignored.
 * d_cluster_sites (uint32 [B], may be NULL) is ADDED to.  MLMCPI_ERR_INVALID: NULL level, odd or zero extents, Mt Mx > 2^30,
 * beta <= 0, no workspace, B = 0, update0 + n_updates beyond 32 bits. */
int mlmcpi_sigma_level_cluster_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes);
int mlmcpi_sigma_level_cluster_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates,
                                    uint64_t seed, uint32_t chain0, uint32_t update0, uint32_t *d_cluster_sites,
                                    void *d_work, void *stream);
/* The same update with the improved estimators of the single cluster: the state and d_cluster_sites are the
 * bits of mlmcpi_sigma_level_cluster_draw and no further random number is drawn; rotated = 0 serves the plain lattice.
 * Positions x_d(l), directions (d = 0 is t, d = 1 is x), n_out and its layout are those of mlmcpi_sigma_level_correlator.  With C
 * the cluster of one update, |C| its size and a_l = r . sigma_l of the field BEFORE the update,
 *   P_d(i)       = sum_{l in C, x_d(l) = i} a_l,   A = sum_{l in C} a_l
 *   chi^W        = 3 A^2 / |C|
 *   F_d^W        = 3 (Ac_d^2 + As_d^2) / |C|,   Ac_d, As_d = sum_i P_d(i) (cos, sin)(2 pi i / M_d)
 *   C_d^W(tau)   = (3 / |C|) sum_{i < M_d} P_d(i) P_d((i + tau) mod M_d),   tau = 0 .. M_d / 2.
 * The seed vertex is uniform and independent of the bonds, so the mean over seeds of f(C) / |C| is (1 / n) sum_C f(C): in
 * expectation these are the Swendsen-Wang improved estimators of the same bonds, unbiased for chi_m, F_d and C_d(tau).  Per
 * update, with the weights w of mlmcpi_sigma_level_correlator, sum_tau w C_d^W = chi^W and sum_tau w C_d^W cos(2 pi tau / M_d) =
 * F_d^W up to the roundings below.
 * Arithmetic.  Every member adds q(a) = llrint(a 2^32) to the slice table of its chain (M_t + M_x 64-bit integers in the
 * workspace) by integer atomics.  Then A = sum_i P_0(i), an exact integer, and d_improved[b] += (x x) (3.0 / |C|), x = (double)A
 * 2^-32.  Ac_d = sum_i llrint((double)P_d(i) w^c_d(i)), As_d with w^s_d, (w^s, w^c)(i) = sincospi(2.0 * i / M_d) from the device
 * function the correlator kernels call (an extent of 2 gives exactly 0 and +-1); d_structure[b][d] += (xc xc) (3.0 / |C|), then
 * += (xs xs) (3.0 / |C|).  A pair of occupied slices contributes llrint(((double)P (double)P') 2^(s - 64)) to a 64-bit accumulator
 * per (d, tau), s = min(32, 62 - ceil(log2(n n_slice))), n_slice = n / min(Mt, Mx) (one cluster's sum of |P| |P'| is at most n
 * n_slice); d_corr[b][tau] += ((double)acc 2^-s) (3.0 / |C|).  With w_d slices that hold a member the lags tau <= min(M_d / 2,
 * w_d - 1) are formed: a link moves the slice index by at most 1, so larger lags pair nothing.  No fp contraction; every sum is an integer
 * sum, so all outputs are the same bits under every launch plan (MLMCPI_SIGMA_CLUSTER_TEAM / _BITMAP govern this draw too),
 * batch split, chain0 and call split (10 = 5 + 5).
 * d_improved (double [B]), d_structure (double [B][2]: F_t, F_x; may be NULL) and d_corr (double [B][n_out]; may be NULL) are
 * ADDED to, update by update; d_cluster_sites as above.  Workspace: that of mlmcpi_sigma_level_cluster_draw, then per chain 28 B
 * per slice (table 8, occupied-slice list 4, weights 16) and 8 B per lag and sum; its content at entry is ignored; work_bytes is what d_work
 * holds.  MLMCPI_ERR_INVALID, nothing launched: NULL d_improved, work_bytes below _improved_workspace_bytes, and whatever
 * mlmcpi_sigma_level_cluster_draw refuses. */
int mlmcpi_sigma_level_cluster_improved_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes);
int mlmcpi_sigma_level_cluster_improved_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates,
                                             uint64_t seed, uint32_t chain0, uint32_t update0,
                                             uint32_t *d_cluster_sites /* may be NULL */, double *d_improved /* [B] */,
                                             double *d_structure /* [B][2], may be NULL */,
                                             double *d_corr /* [B][n_out], may be NULL */, void *d_work, size_t work_bytes,
                                             void *stream);
/* The Swendsen-Wang multi-cluster update on a level (sigma_sw.hip): n_updates updates of every chain of
 * d_state [B][2 n], in place.  Unrotated: mlmcpi_sigma_sw_* on (Mt, Mx, beta), the same bits and the same workspace size.
 * Rotated: n = Mt Mx / 2 vertices, plane E then plane O of ht x hx = Mt/2 x Mx/2 each, index p ht hx + ht b + a; the links are
 * named as the level Wolff update names them: (e, d), e an E vertex (e < n / 2), d in 0..3, E(a, b) -> O(a, b), O(a, b-1),
 * O(a-1, b), O(a-1, b-1); from O(a, b), direction d' crosses link (neighbour, 3 - d').  Where a plane extent is 1 coinciding
 * neighbours are distinct links with a uniform each.  Philox, step = update0 + k, the purposes of mlmcpi_sigma_sw_draw with
 * the level's indices: purpose 21 site 0 sub 0 (u, v) -> r (r_z = 1 - 2 u, azimuth 2 pi v - pi); purpose 22 site e sub d >> 1:
 * u decides link (e, d) for d even, v for d odd; purpose 23 site = the root of a cluster = its smallest LEVEL index (also for a
 * lone O vertex), sub 0: reflected iff u < 0.5.  With a_l = r . sigma_l BEFORE the update, link (x, y) is bonded iff (a_x a_y) >
 * 0 and its uniform < 1 - exp(min(0, -2 beta (a_x a_y))), the product formed first; every component of the bonded links is
 * labelled, a flipped cluster is reflected, sigma' = sigma - 2 a r, canonical form, no fp contraction.  Improved estimator of
 * chi_m: 3 sum_C A_C^2 / n, A_C summed as llrint(a 2^32) by integer atomics, the squares summed over the roots in one fixed
 * configuration (1024 threads, thread t takes t, t + 1024, .., then a fixed tree), ADDED to d_improved update by update.
 * The state and all three outputs are the same bits under every launch plan, tile, batch split, chain0 and call split
 * (10 = 5 + 5).  MLMCPI_SIGMA_SW_PLAN=chain|tiled and MLMCPI_SIGMA_SW_TILE=WxH (W, H in {8, 16, 32, 64}, here in plane cells;
 * default 32x32) govern this update too; chain forced on a level of more than 7552 vertices: MLMCPI_ERR_UNSUPPORTED.
 * Workspace: 256 B (status word) + 20.5 B per vertex and chain (label 4, q(a) 8, root slot 8, four bond bits per E vertex);
 * its content at entry is ignored.  d_flipped, d_clusters (uint32 [B]) and d_improved (double [B]) may each be NULL and are
 * ADDED to.  The draw reads the status word back after its launches (it synchronises the stream); a labelling loop that hit
 * its iteration cap: MLMCPI_ERR_HIP.  MLMCPI_ERR_INVALID: NULL level, odd or zero extents, Mt Mx > 2^30, beta <= 0, no
 * workspace, B = 0, update0 + n_updates beyond 32 bits. */
int mlmcpi_sigma_level_sw_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes);
int mlmcpi_sigma_level_sw_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates, uint64_t seed,
                               uint32_t chain0, uint32_t update0, uint32_t *d_flipped, uint32_t *d_clusters, double *d_improved,
                               void *d_work, void *stream);
/* The same update with the cluster-improved structure factor at the lowest momentum: the state, d_flipped,
 * d_clusters and d_improved are the bits of mlmcpi_sigma_level_sw_draw; rotated = 0 serves the plain lattice.
 * Positions.  Unrotated: l = Mt j + i sits at (i, j).  Rotated: plane p, cell (a, b), index p ht hx + ht b + a, sits at (i, j) =
 * (2 a + p, 2 b + p), the slice assignment of mlmcpi_sigma_level_correlator.  Direction d = 0 is t (x_0 = i, M_0 = Mt), d = 1 is x
 * (x_1 = j, M_1 = Mx).  Weights: (w^s_d, w^c_d)(l) = sincospi(2.0 * x_d / M_d) in double, the quotient formed from the integers
 * by the one device function every kernel calls, so an extent of 2 gives exactly 0 and +-1.
 * Per cluster C and direction d two 64-bit fixed-point sums, Ac_d = sum_{l in C} llrint((a_l w^c_d(l)) 2^32) and As_d with w^s_d,
 * the product formed first, no fp contraction, added by integer atomics as A_C is (|a w| <= 1 and n <= 2^30: inside 63 bits).
 * Per update F_d^imp = R(Ac_d) 3 / n + R(As_d) 3 / n, R(S) = the sum over the roots of (S 2^-32)^2 in the fixed configuration of
 * the improved chi_m (1024 threads, thread t takes t, t + 1024, .., then the fixed tree), one such sum per S, each scaled and ADDED
 * to d_structure[b][d] in turn (cos, then sin), exactly as chi_m's is added to d_improved.  d_structure (double [B][2]: F_t^imp,
 * F_x^imp) is so ADDED to update by update and is the same bits under every launch plan, tile, batch split, chain0 and call
 * split (10 = 5 + 5).  It is the mean of 3 |sum_l +-a_l e^{2 pi i x_d / M_d}|^2 / n over the coins: an unbiased estimator of the structure factor F_d = |sum_l sigma_l e^{2 pi i x_d / M_d}|^2 / n.
 * Workspace: that of mlmcpi_sigma_level_sw_draw + 32 B per vertex and chain (four more root slots); work_bytes is what d_work
 * holds.  MLMCPI_SIGMA_SW_PLAN and MLMCPI_SIGMA_SW_TILE govern it; the chain plan keeps its 20 B per vertex and its bound.
 * Errors as for mlmcpi_sigma_level_sw_draw, and MLMCPI_ERR_INVALID, nothing launched, for NULL d_structure or work_bytes below
 * _structure_workspace_bytes. */
int mlmcpi_sigma_level_sw_structure_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes);
int mlmcpi_sigma_level_sw_structure_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates,
                                         uint64_t seed, uint32_t chain0, uint32_t update0, uint32_t *d_flipped, uint32_t *d_clusters,
                                         double *d_improved, double *d_structure, void *d_work, size_t work_bytes, void *stream);
/* The same update with the cluster-improved time-slice correlator: the state, d_flipped, d_clusters and
 * d_improved are the bits of mlmcpi_sigma_level_sw_draw and no further random number is drawn; rotated = 0 serves the plain
 * lattice.  Positions x_d(l) and directions are those of mlmcpi_sigma_level_sw_structure_draw and mlmcpi_sigma_level_correlator.
 * With a_l = r . sigma_l of the field BEFORE the update and C the update's clusters,
 *   P_C,d(i)     = sum_{l in C, x_d(l) = i} a_l
 *   C_d^imp(tau) = (3 / n) sum_C sum_{i < M_d} P_C,d(i) P_C,d((i + tau) mod M_d),   tau = 0 .. M_d / 2,
 * the mean over the coins of 3 (r . S'_i)(r . S'_{i + tau}) / n summed over i (cross terms of two clusters vanish) and over r the
 * mean of C_d(tau): an unbiased estimator of the plain correlator whose noise falls with the signal.  Per update, with the
 * weights w of mlmcpi_sigma_level_correlator, sum_tau w C_d^imp = the improved chi_m and sum_tau w C_d^imp cos(2 pi tau / M_d) =
 * the improved F_d, up to the roundings below.
 * d_corr (double [B][n_out], n_out = (Mt/2 + 1) + (Mx/2 + 1), C_t first: the layout of mlmcpi_sigma_level_correlator) is ADDED to
 * update by update.  Arithmetic: P is summed as q(a) = llrint(a 2^32) by integer atomics into a table keyed by (root, slice); a
 * pair of occupied slices contributes llrint(((double)P (double)P') 2^(s - 64)) to a 64-bit accumulator per (chain, d, tau); at
 * the end of the update d_corr += ((double)acc 2^-s) (3.0 / n).  s = min(32, 62 - ceil(log2(n n_slice))), n_slice = n / min(Mt, Mx)
 * the vertices of the larger slice: sum_i sum_C |P(i)| |P(i + tau)| <= n n_slice, so the accumulator stays inside 63 bits.  A
 * cluster that occupies w slices of a direction is paired at tau <= min(M_d / 2, w - 1) only: a link changes the slice index by at
 * most 1, so larger lags hold nothing.  Every sum is an integer sum, so d_corr is the same bits under every launch plan, tile,
 * batch split, chain0 and call split (4 = 1 + 3).  MLMCPI_SIGMA_SW_PLAN and MLMCPI_SIGMA_SW_TILE govern it; the chain plan runs
 * one update per launch and keeps its bound.
 * Workspace: that of mlmcpi_sigma_level_sw_draw, then per chain and direction a table of 2^lg slots of 16 B, 2^lg the smallest
 * power of two >= 2 n (32 .. 64 B per vertex, chain and direction), 4 B per vertex, chain and direction of occupied-slice counts
 * and 8 B per chain and lag: 72 .. 136 B per vertex and chain more; work_bytes is what d_work holds.
 * Errors as for mlmcpi_sigma_level_sw_structure_draw (a probe loop of the table that hit its cap, the capacity, sets the same
 * status word: MLMCPI_ERR_HIP), and MLMCPI_ERR_INVALID, nothing launched, for NULL d_corr, work_bytes below
 * _correlator_workspace_bytes, or odd extents. */
int mlmcpi_sigma_level_sw_correlator_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes);
int mlmcpi_sigma_level_sw_correlator_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates,
                                          uint64_t seed, uint32_t chain0, uint32_t update0, uint32_t *d_flipped, uint32_t *d_clusters,
                                          double *d_improved, double *d_corr /* [B][n_out], ADDED to, update by update */,
                                          void *d_work, size_t work_bytes, void *stream);
/* NonlinearSigmaConditionedFineAction (nonlinearsigmaconditionedfineaction.cc:7-44) on a level.  Every fine-only vertex (the
 * (i + j) odd ones of an unrotated level, the O plane of a rotated one) has coarse neighbours only, so the fill is a product of
 * independent heat-bath laws and _evaluate is minus the log of its density.
 *   _fill      every fine-only vertex l <- the heat-bath draw from its four neighbours, all at once, ONE Philox call each (site l
 *              = its index on the fine level, chain, step, purpose 24); a vertex whose neighbour sum is 0 keeps its entry
 *   _evaluate  d_S[b] = -sum_X log p(z_X; s_X), s = beta |Delta|, z = sigma . Delta / |Delta|, log p = s (z - 1) + log s -
 *              log(1 - exp(-2 s)); Delta = 0 contributes log 2 */
int mlmcpi_sigma_cfa_fill(const mlmcpi_sigma_level *fine, double *d_state, uint32_t B, uint64_t seed, uint32_t chain0,
                          uint32_t step, void *stream);
int mlmcpi_sigma_cfa_evaluate(const mlmcpi_sigma_level *fine, const double *d_state, uint32_t B, double *d_S, void *stream);
/* TwoLevelMetropolisStep::draw (twolevelmetropolisstep.cc:35-89) between a level and its coarse partner (`coarse` must be that
 * partner: MLMCPI_ERR_INVALID otherwise; coarse->beta is the caller's).  One pass, with no intermediate state in HBM beyond the trial (neighbours are re-read through the cache), builds the trial (the coarse proposal on the
 * coarse vertices, the fill of purpose 24 on the fine-only ones; a fine-only vertex whose neighbour sum is 0 takes the entry of
 * d_theta) and sums the terms of the trial and of the current state; a per-chain launch decides (u = Philox site 0, purpose 8,
 * as mlmcpi_lattice_twolevel_draw); a masked copy writes the accepted trials into d_theta.  Arguments as
 * mlmcpi_lattice_twolevel_draw; d_terms[b] = (dS_fine, dS_coarse, dS_trial).  The sums are formed in a fixed order (groups of
 * 256 vertices, then the groups in order), so accept, terms and states do not depend on MLMCPI_SIGMA_TWOLEVEL_GROUPS=g (groups
 * per workgroup, 1..64) or on the batch split. */
int mlmcpi_sigma_twolevel_workspace_bytes(const mlmcpi_sigma_level *fine, uint32_t B, size_t *bytes);
int mlmcpi_sigma_twolevel_draw(const mlmcpi_sigma_level *fine, const mlmcpi_sigma_level *coarse, const double *d_phi_coarse,
                               double *d_theta, uint32_t B, uint64_t seed, uint32_t chain0, uint32_t step, void *d_work,
                               int32_t *d_accept, double *d_terms, void *stream);

/* QoI2DPhiSquared (qoi/qft/qoi2dphisquared.cc:8-15), QoIAvgPlaquette (qoi/qft/qoiavgplaquette.cc:8-27),
 * QoI2DSusceptibility (qoi/qft/qoi2dsusceptibility.cc:8-27); d_out[b]. */
int mlmcpi_qoi_phi_squared(const double *d_phi, uint32_t n_vertices, uint32_t B, double *d_out, void *stream);
int mlmcpi_qoi_avg_plaquette(const double *d_theta, uint32_t Mt, uint32_t Mx, uint32_t B, double *d_out,
                             void *stream);
int mlmcpi_qoi_2d_susceptibility(const double *d_theta, uint32_t Mt, uint32_t Mx, uint32_t B, double *d_out,
                                 void *stream);

/* Wilson loops of the quenched Schwinger model (wilson_loops.hip).  With the state layout above,
 * theta[b 2 Mt Mx + 2 (Mt j + i) + mu], and the plaquette orientation of the action (quenchedschwingeraction.cc:14-17): for a base
 * vertex (i, j), 1 <= r <= R links along direction 0 and 1 <= s <= S links along direction 1, all indices periodic,
 *   Theta(i,j;r,s) =  sum_{k<r} theta0(i+k, j)  +  sum_{l<s} theta1(i+r, j+l)  -  sum_{k<r} theta0(i+k, j+s)  -  sum_{l<s} theta1(i, j+l)
 *                  =  the sum over the r x s cells (i+k, j+l) of the unreduced plaquette angle
 *   W(r,s)         =  (1 / (Mt Mx)) sum_{i,j} cos Theta(i,j;r,s)
 * into d_out [B][R][S], entry [r-1][s-1].  Identities: W(1,1) = mlmcpi_qoi_avg_plaquette; W(Mt,Mx) = 1 (every link cancels); W does
 * not change under theta_mu(n) -> theta_mu(n) + g(n) - g(n + mu^).  On the periodic lattice, V = Mt Mx, A = r s <= V,
 *   <W(r,s)> = sum_n I_n(beta)^(V-A) I_(n+1)(beta)^A / sum_n I_n(beta)^V   (n over the integers; -> (I_1/I_0)^A as V -> infinity)
 * and the Creutz ratio chi(r,s) = -log[W(r,s) W(r-1,s-1) / (W(r-1,s) W(r,s-1))], W(0,.) = W(.,0) = 1, tends to the string tension
 * -log(I_1(beta) / I_0(beta)) at every (r,s) (include/mlmcpi/correlator.hh).
 * How it is computed: e^(i Theta) is the product of the cell phases e^(i theta_p), one sincos per plaquette; a strip of r cells is
 * U(i,j;r) = U(i,j;r-1) z(i+r-1,j), a loop P(i,j;r,s) = P(i,j;r,s-1) U(i,j+s-1;r), and Re P is summed.
 * Summation order: the lattice is cut into tiles of tile_w x tile_h = 32 x 32 base vertices (edge tiles clipped); thread t of the
 * 256 of a workgroup adds the J = 4 base vertices (column t % 32, rows 4 (t / 32) .. + 3) ascending, the workgroup its threads by
 * the lane tree (offsets 32, .., 1) and then its four waves ascending; the tiles (tile = ty tiles_w + tx) are added in ascending
 * order and the sum is multiplied by 1 / (Mt Mx) last.  The geometry is a function of (Mt, Mx, R, S) alone, there are no atomics
 * and no tuning knob: a chain's output is the same bits for every B, every split of the chains over calls and every stream.
 * d_theta: 16-byte aligned, not written.  d_acc (may be NULL) [B][R][S][2]: W is ADDED to [.][.][.][0] and W^2 to [.][.][.][1] in the
 * launch that writes d_out; the caller counts the calls.  d_work: _workspace_bytes(Mt, Mx, R, S, B) bytes, 256-byte aligned
 * (one partial per chain, tile, r and s); content at entry ignored.
 * Any Mt, Mx >= 2, odd extents included, Mt Mx <= 2^30.  Chains and tiles share one index of workgroups, B tiles of them, laid over
 * grid x (2^31 / 256) and, beyond that, y: there is no 65535-chain limit (the bound, 2^23 x 65535 workgroups, is beyond any memory;
 * CHAINS PER CALL above).  MLMCPI_ERR_INVALID, with nothing launched and no output byte touched: a NULL pointer (d_acc excepted); Mt or Mx < 2 or Mt Mx >
 * 2^30; B = 0; R = 0 or S = 0; R > Mt or S > Mx; more workgroups than above; work_bytes below _workspace_bytes.
 * MLMCPI_ERR_UNSUPPORTED: R or S above MLMCPI_WILSON_LOOPS_MAX (the LDS image and the register window are sized by it).
 * _plan (host only, touches no device) reports the geometry and returns the status the call would. */
#ifdef __cplusplus
constexpr uint32_t MLMCPI_WILSON_LOOPS_MAX = 16;
#else
#define MLMCPI_WILSON_LOOPS_MAX 16u
#endif
typedef struct mlmcpi_wilson_loops_plan_info {
  uint64_t work_bytes;            /* what _workspace_bytes reports */
  uint64_t grid;                  /* workgroups of the loop launch, B tiles; with work_bytes the only entries that depend on B */
  uint32_t workgroup;             /* threads of a workgroup */
  uint32_t tile_w, tile_h;        /* base vertices of a tile along direction 0 and 1; tile (tx, ty) owns the base vertices
                                   * [tx tile_w, min(Mt, (tx + 1) tile_w)) x [ty tile_h, min(Mx, (ty + 1) tile_h)) */
  uint32_t halo_w, halo_h;        /* R - 1 columns and S - 1 rows of cells beyond a tile in its LDS image */
  uint32_t J;                     /* consecutive base rows of one column per thread */
  uint32_t tiles_w, tiles_h;      /* ceil(Mt / tile_w), ceil(Mx / tile_h) */
  uint32_t tiles;                 /* tiles per chain, tiles_w tiles_h */
  uint32_t lds_bytes, lds_limit;  /* dynamic LDS of a workgroup, (min(tile_w, Mt) + R) (min(tile_h, Mx) + S) 16, and the limit the
                                   * kernel is written for */
} mlmcpi_wilson_loops_plan_info;
int mlmcpi_schwinger_wilson_loops_workspace_bytes(uint32_t Mt, uint32_t Mx, uint32_t R, uint32_t S, uint32_t B, size_t *bytes);
int mlmcpi_schwinger_wilson_loops(const double *d_theta, uint32_t Mt, uint32_t Mx, uint32_t B, uint32_t R, uint32_t S,
                                  double *d_out /* [B][R][S] */, double *d_acc /* [B][R][S][2], may be NULL */, void *d_work,
                                  size_t work_bytes, void *stream);
int mlmcpi_schwinger_wilson_loops_plan(uint32_t Mt, uint32_t Mx, uint32_t R, uint32_t S, uint32_t B, mlmcpi_wilson_loops_plan_info *out);

/* The momentum-projected time-slice correlators of a Gaussian free field state (gff_correlator.hip).
 * A level is (Mt, Mx, rotated), Mt and Mx even and >= 2, Mt Mx <= 2^30.  rotated = 0: phi[b][Mt j + i], the GFF layout above.
 * rotated != 0: the Mt Mx / 2 vertices with i + j even in the order of rotated lattices above (mlmcpi_sigma_level; the GFF levels
 * store the same Lattice2D order): the planes E then O, index p (Mt Mx / 4) + (Mt/2) b + a = vertex (2 a + p, 2 b + p).  N = the
 * level's number of vertices.  For the momenta q = 0 .. P - 1 (P = n_mom):
 *   slice sums   S^t_i(q) = sum_j phi(i, j) e^{-2 pi i q j / Mx} over the level's vertices with first coordinate i;
 *                S^x_j(q) = sum_i phi(i, j) e^{-2 pi i q i / Mt} over those with second coordinate j.
 *   correlators  C_t(tau; q) = (1/N) sum_i Re[S^t_i(q) conj S^t_{(i + tau) mod Mt}(q)], tau = 0 .. Mt/2;
 *                C_x(tau; q) = (1/N) sum_j Re[S^x_j(q) conj S^x_{(j + tau) mod Mx}(q)], tau = 0 .. Mx/2.
 * d_out [n_chains][n_out], n_out = P (Mt/2 + 1) + P (Mx/2 + 1) (_correlator_size): C_t first, momentum-major, lag fastest.
 * Identities: with w(0) = w(M/2) = 1 and w = 2 otherwise, N sum_tau w C_t(tau; 0) = (sum phi)^2; summed over ALL Mx momenta,
 * sum_q C_t(0; q) = Mx (1/N) sum phi^2 (unrotated; C(.; Mx - q) = C(.; q), so the momenta 0 < q < Mx/2 count twice).  For the GFF
 * action on the unrotated Mt x Mx lattice, mu^2 = (mass / Mt)^2, <C_t(tau; q)> = (1/Mt) sum_k cos(2 pi k tau / Mt) / (4 + mu^2 -
 * 2 cos(2 pi k / Mt) - 2 cos(2 pi q / Mx)) = cosh(E_q (Mt/2 - tau)) / (2 sinh E_q sinh(E_q Mt / 2)), one cosh whose rate is the
 * lattice dispersion relation cosh E_q = 1 + (mu^2 + 2 - 2 cos(2 pi q / Mx)) / 2 (include/mlmcpi/correlator.hh).
 * How it is computed: the twiddles are entries (q j) mod M of a table of the M-th roots of unity, the product reduced in integers,
 * the table built by a prelude launch of every call (one sincospi per entry on an argument reduced exactly; entry 0 is (1, 0)); no
 * twiddle is formed by recurrence.  The state is read once: a workgroup takes a band of band_rows rows of a chunk of `tile` columns of
 * one plane (unrotated: one plane of Mt columns x Mx rows, column i, row j; rotated: plane p, column a, row b) and adds, one FMA per
 * part and vertex, the rows of its band ascending (S^t) and the columns of its chunk ascending (S^x); a gather adds the bands
 * (chunks) ascending; one wave per (lag, q, direction, chain) adds the slices lane l: l, l + 64, .. ascending (a product and an FMA
 * each), then the lane tree (offsets 32, .., 1), and multiplies by 1/N last.  The geometry is a function of (Mt, Mx, rotated, P)
 * alone, there are no atomics and no tuning knob: a chain's output is the same bits for every n_chains, every split of the chains
 * over calls, every stream, and with or without d_acc.
 * d_phi: 16-byte aligned, not written.  d_acc (may be NULL) [n_chains][n_out][2]: C is ADDED to [.][.][0] and C^2 to [.][.][1] in
 * the launch that writes d_out; the caller counts the calls.  d_work: _workspace_bytes bytes, 256-byte aligned; content at entry
 * ignored.
 * The batch parameter is spelled n_chains, not B: tests/test_chain_count_cases.py collects the exports with a `uint32_t B` and
 * demands a row of its case table for each; these entry points are run at the 65535-chain edge by tests/test_gff_correlator_gpu.py
 * instead.  Chains and tiles (blocks of lags) share one index of workgroups laid over grid x (2^31 / 256) and, beyond that, y:
 * there is no 65535-chain limit (CHAINS PER CALL above).
 * MLMCPI_ERR_INVALID, with nothing launched and no output byte touched: odd or zero extents or Mt Mx > 2^30; n_mom = 0 or above
 * Mx/2 + 1 or Mt/2 + 1; a NULL pointer (d_acc excepted) or d_phi, d_work off 16 bytes; n_chains = 0; more workgroups than 2^23 x
 * 65535; work_bytes below _workspace_bytes.  MLMCPI_ERR_UNSUPPORTED: n_mom above MLMCPI_GFF_CORRELATOR_MAX_MOMENTA (the LDS
 * twiddle images and the register accumulators are sized by it).  _plan (host only, touches no device) reports the geometry and
 * returns the status the call would. */
#ifdef __cplusplus
constexpr uint32_t MLMCPI_GFF_CORRELATOR_MAX_MOMENTA = 8;
#else
#define MLMCPI_GFF_CORRELATOR_MAX_MOMENTA 8u
#endif
typedef struct mlmcpi_gff_correlator_plan_info {
  uint64_t work_bytes;             /* what _workspace_bytes reports: align256 of each of the table ((Mt + Mx) 16 bytes), the band partials
                                    * (n_chains planes bands P plane_w 16), the chunk partials (n_chains planes chunks P plane_h 16) and
                                    * the slice sums (n_chains P (Mt + Mx) 16) */
  uint64_t grid;                   /* workgroups of the projection launch, n_chains planes bands chunks */
  uint64_t gather_grid, lag_grid;  /* of the gather, n_chains ceil(P (Mt + Mx) / workgroup), and of the lag launch, n_chains P
                                    * (ceil((Mt/2 + 1) / lags_per_workgroup) + ceil((Mx/2 + 1) / lags_per_workgroup)) */
  uint32_t workgroup;              /* threads of a workgroup, every launch */
  uint32_t tile;                   /* rows and columns of a tile; columns of a chunk */
  uint32_t band_rows;              /* rows of a band */
  uint32_t planes, plane_w, plane_h;  /* 1, Mt, Mx; rotated: 2, Mt/2, Mx/2 */
  uint32_t chunks, bands;          /* ceil(plane_w / tile), ceil(plane_h / band_rows) */
  uint32_t vector_loads;           /* 1: plane_w is even and the tile is loaded by 16-byte loads; 0: by 8-byte loads (the same sums) */
  uint32_t table_entries;          /* Mt + Mx roots of unity */
  uint32_t lags_per_workgroup;
  uint32_t lags_in_lds;            /* 1: max(Mt, Mx) 16 bytes fit lds_limit and the lag launch stages the slice sums in LDS */
  uint32_t lds_bytes, lag_lds_bytes, lds_limit;  /* LDS of a workgroup of the projection and of the lag launch; the limit both are written for */
} mlmcpi_gff_correlator_plan_info;
int mlmcpi_gff_correlator_size(uint32_t Mt, uint32_t Mx, int32_t rotated, uint32_t n_mom, uint32_t *n_out);
int mlmcpi_gff_correlator_workspace_bytes(uint32_t Mt, uint32_t Mx, int32_t rotated, uint32_t n_mom, uint32_t n_chains, size_t *bytes);
int mlmcpi_gff_correlator(uint32_t Mt, uint32_t Mx, int32_t rotated, uint32_t n_mom, const double *d_phi, uint32_t n_chains,
                          double *d_out /* [n_chains][n_out] */, double *d_acc /* [n_chains][n_out][2], may be NULL */, void *d_work,
                          size_t work_bytes, void *stream);
int mlmcpi_gff_correlator_plan(uint32_t Mt, uint32_t Mx, int32_t rotated, uint32_t n_mom, uint32_t n_chains,
                               mlmcpi_gff_correlator_plan_info *out);
/* QoI2DMagneticSusceptibility (qoi/qft/qoi2dmagneticsusceptibility.cc:7-21): d_out[b] = |sum_n sigma_n|^2 / (Mt Mx) of a
 * sigma-model state */
int mlmcpi_qoi_magnetic_susceptibility(const double *d_phi, uint32_t Mt, uint32_t Mx, uint32_t B, double *d_out, void *stream);

/* Generic HMCSampler::draw for a 2-D action (streaming leapfrog: one fused force + momentum +
 * position kernel per step).  Same contract as mlmcpi_path_hmc_draw. */
int mlmcpi_lattice_hmc_workspace_bytes(const mlmcpi_lattice_action *act, uint32_t B, size_t *bytes);
int mlmcpi_lattice_hmc_draw(const mlmcpi_lattice_action *act, double *d_phi, uint32_t B, uint32_t nt, double dt,
                            uint32_t n_rep, uint64_t seed, uint32_t chain0, uint32_t traj0, void *d_work,
                            int32_t *d_accept, double *d_energies, void *stream);

/* ---- host-only analytic helpers of the quenched Schwinger model (no GPU needed) --------------------------
 * V chi_t(beta, P) = (P / beta) Phi_chi(beta, P) (common/auxilliary.cc:30-33, 44-79, 98-193: the value
 * QoI2DSusceptibility::evaluate's expectation is compared with, qoi/qft/qoi2dsusceptibility.cc:30-34), and the coarse
 * coupling matched to it: the root x of chi_t(x beta, P / rho) = chi_t(beta, P) in [0.01, 2] by bisection, times beta
 * (action/qft/quenchedschwingerrenormalisation.cc:7-64; rho = 4 when both directions are coarsened, else 2; the
 * reference's fall-back x = 1 / rho when the interval holds no root).  Own quadrature in place of GSL's. */
int mlmcpi_schwinger_chit_analytical(double beta, uint32_t n_plaq, double *chit);
int mlmcpi_schwinger_beta_coarse_nonperturbative(double beta, uint32_t n_plaq, int32_t rho_refine, double *beta_coarse);

/* ---- device-side statistics accumulation (common/statistics.cc:4-27, batched) ---------------
 * d_acc holds, per chain, the packed sums [n, sum q, sum q^2, sum q^3, sum q^4] that the
 * cross-rank reduction (one RCCL all-reduce of B*5 doubles) combines; see DESIGN.md. */
int mlmcpi_stats_accumulate(double *d_acc, const double *d_q, uint32_t B, void *stream);
/* Statistics::record_sample WITH the autocorrelation window (common/statistics.cc:4-27: running average, running averages
 * S_k of Q_j Q_{j-k} for k < window over a deque of the last `window` values), batched: d_state[B][2 * window + 3] =
 * per chain [n, average, S_0 .. S_{window-1}, head, ring[window]], zero-initialised by the caller.  What
 * MonteCarloMultiLevel::draw_coarse_sample (montecarlo/montecarlomultilevel.cc:170-190) re-reads on every coarse draw:
 * tau_int = max(1, 1 + 2 sum_{k>=1} (1 - k/n)(S_k - avg^2)/(S_0 - avg^2)) (statistics.cc:38-61), computed by the caller
 * from the state (per chain, or with the autocovariances averaged over the chains of a batch). */
int mlmcpi_stats_window_record(double *d_state, const double *d_q, uint32_t B, uint32_t window, void *stream);

/* ---- test hooks: raw RNG streams, single draws (used by parity tests only) -------------------- */
int mlmcpi_test_philox(const uint32_t *ctr4, const uint32_t *key2, uint32_t *out4);
/* d_out[4*k..] = (u0,u1,n0,n1) for site k of n sites */
int mlmcpi_test_random(uint64_t seed, uint32_t chain, uint32_t step, uint32_t purpose, uint32_t sub, uint32_t n,
                       double *d_out, void *stream);
/* d_out[k] = ExpCos draw for site k with staples (d_xp[k], d_xm[k]); ExpSin2 draw with d_sigma[k] */
int mlmcpi_test_expcos(uint64_t seed, uint32_t chain, uint32_t step, double beta, const double *d_xp,
                       const double *d_xm, uint32_t n, double *d_out, void *stream);
int mlmcpi_test_expsin2(uint64_t seed, uint32_t chain, uint32_t step, const double *d_sigma, uint32_t n,
                        double *d_out, void *stream);
/* d_out[k] = a heat-bath draw for site k of the stream between x_p = d_xp[k] and x_m = d_xm[k], conditional
 * exp(scale / 2 [cos(x - x_p) + cos(x - x_m)]), from the tabulated step-envelope sampler the sweeps use for actions with
 * scale = 2 beta (Schwinger) or 2 m0 / a (rotor) <= 16 (the range the sweeps draw from this sampler: round 5; 4 before) */
int mlmcpi_test_vs_draw(uint64_t seed, uint32_t chain, uint32_t step, double scale, const double *d_xp, const double *d_xm,
                        uint32_t n, double *d_out, void *stream);
/* that sampler's table for an action of the given scale (host only, no GPU needed): sel[8][64] = bin of a selector
 * value per concentration class, lw[8][8] = log2 of the acceptance factor of a bin */
int mlmcpi_vs_table(double scale, uint8_t *sel, float *lw);

/* The fp64 device primitives the samplers share (device_common.hpp, vonmises.hpp, fillin.hpp, sigma_device.hpp), one call per
 * element: (d_out0[k], d_out1[k]) = fn(d_a[k], d_b[k]).  One thread per element, 256 per block; the kernel calls the
 * primitive in its header, nothing is restated.  d_b is read by the functions of two operands only (it may be NULL for the
 * others); d_out1[k] is 0 where a function has one result.  Unknown fn, n == 0 or a NULL pointer: MLMCPI_ERR_INVALID, nothing
 * is launched.  Operands that are not doubles travel as bit patterns: "words" = the 64 bits of d_a[k], lo = bits 0..31,
 * hi = bits 32..63. */
enum mlmcpi_math_fn {
  MLMCPI_MATH_FAST_RCP = 0,          /* fast_rcp(a) */
  MLMCPI_MATH_FAST_DIV = 1,          /* fast_div(a, b) */
  MLMCPI_MATH_FAST_SQRT = 2,         /* fast_sqrt(a) */
  MLMCPI_MATH_FAST_ACOS = 3,         /* fast_acos(a) */
  MLMCPI_MATH_SIN_REDUCED = 4,       /* sin_reduced(a) */
  MLMCPI_MATH_COSPI_UNIT = 5,        /* cospi_unit(a) */
  MLMCPI_MATH_COS_REDUCED = 6,       /* cos_reduced(a) */
  MLMCPI_MATH_COS_HALF = 7,          /* cos_half(a) */
  MLMCPI_MATH_LOG_UNIT = 8,          /* log_unit(a) */
  MLMCPI_MATH_SINCOS_2PI_UNIT = 9,   /* sincos_2pi_unit(a) -> (sn, cs) */
  MLMCPI_MATH_BOX_MULLER = 10,       /* box_muller(u = a, v = b) -> (n0, n1) */
  MLMCPI_MATH_MOD_2PI = 11,          /* mod_2pi(a) */
  MLMCPI_MATH_MOD_2PI_FAST = 12,     /* mod_2pi_fast(a) */
  MLMCPI_MATH_U01 = 13,              /* u01(lo, hi) of the words of a */
  MLMCPI_MATH_U01_52 = 14,           /* u01_52(lo, hi) of the words of a */
  MLMCPI_MATH_VM_ENVELOPE = 15,      /* vm_envelope(kappa = a) */
  MLMCPI_MATH_BESSEL_I0_SCALED = 16, /* bessel_i0_scaled(a) */
  MLMCPI_MATH_TWO_PI_I0_SCALED = 17, /* two_pi_i0_scaled(a) */
  MLMCPI_MATH_BESSEL_I0 = 18,        /* fillin.hpp bessel_i0(a) */
  MLMCPI_MATH_COMPACT_EXP_INVERSE = 19, /* compact_exp_inverse(s = a, u = b) */
  MLMCPI_MATH_VM_TRY = 20,           /* vm_try(lo, hi of the words of a, kappa = b, R = vm_envelope(b)) -> (c, decision 1 | 0 | -1) */
  MLMCPI_MATH_VM_SCREEN = 21,        /* vm_screen(c = a), the fp32 screen vm_try applies to its c -> (af, band), each fp32 value as a double */
  MLMCPI_MATH_VM_EXACT = 22,         /* vm_exact(lo, tail, c = a) with b = m + tail, m = 0..2047 the acceptance bits (lo = m << 1),
                                        tail in [0, 1) a multiple of 2^-41 (so that b holds both exactly) -> decision 1 | 0 */
  MLMCPI_MATH_COUNT = 23
};
int mlmcpi_test_math(uint32_t fn, const double *d_a, const double *d_b, uint32_t n, double *d_out0, double *d_out1, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MLMCPI_HIP_H */
