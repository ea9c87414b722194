// path_hmc.hip -- fused HMC for the 1-D paths: state AND momenta stay in registers for the whole trajectory, one workgroup
// per chain segment, halo of nt+1 sites recomputed redundantly, so HBM sees one read and one write of the path per
// trajectory instead of 4 x 8 B per site per leapfrog step; whole chains in one launch where the path fits a workgroup.
#include "path_common.hpp"

namespace mlmcpi {

// ---- what the two kernels below share: the leapfrog loop and the Metropolis decision.  Momentum staging and the energy sums
// stay written out in each: shared, they cost hmc_chain_kernel<., 8 | 16> 7 to 25 VGPRs (128 -> 137 for <0, 8>: a wave less per SIMD).
// sampler/hmcsampler.cc:22-57: nt+1 force evaluations with half steps for p at both ends and no position update after the
// last.  exchange() refreshes xl / xr, the neighbours of x[0] and x[R-1], from the new positions.
template <int KIND, int R, class Exchange>
__device__ __forceinline__ void leapfrog(const PathP &P, double (&x)[R], double (&p)[R], double &xl, double &xr, uint32_t nt,
                                         double dt, Exchange exchange) {
  for (uint32_t k = 0; k <= nt; ++k) {
    const double dtp = (k == 0 || k == nt) ? 0.5 * dt : dt;
    const double dtx = (k == nt) ? 0.0 : dt;
    if (KIND == MLMCPI_ROTOR) {
      // one sine per link: d_r = sin(x_r - x_{r-1}); F_r = c1 (d_r - d_{r+1}), identical to
      // c1 (sin(x-x_m) + sin(x-x_p)) because sin is odd
      double dprev = sin_reduced(x[0] - xl);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double dnext = sin_reduced((r == R - 1 ? xr : x[r + 1]) - x[r]);
        p[r] -= dtp * (P.c1 * (dprev - dnext));
        dprev = dnext;
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      double left = xl;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double right = (r == R - 1) ? xr : x[r + 1];
        const double f = site_force<KIND>(P, left, x[r], right);
        left = x[r];
        p[r] -= dtp * f;
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) x[r] += dtx * p[r];
    if (k < nt) exchange();  // positions do not change in the last step: xl stays valid
  }
}

// Metropolis test of one trajectory from its four raw sums S_cur, T0, S_trial, T1 (sampler/hmcsampler.cc:50-67); the chain's
// P_ACCEPT uniform is drawn only where dH >= 0.  energies_b != NULL: S0, T0, S1, T1 go there.
__device__ __forceinline__ bool hmc_decide(const RngKey &key, double escale, const double (&sums)[4], double *energies_b) {
  const double S0 = escale * sums[0], T0 = 0.5 * sums[1], S1 = escale * sums[2], T1 = 0.5 * sums[3];
  const double dH = (S1 - S0) + (T1 - T0);
  if (energies_b) {
    energies_b[0] = S0; energies_b[1] = T0; energies_b[2] = S1; energies_b[3] = T1;
  }
  if (dH < 0.0) return true;
  double u, v;
  rng_uniforms(key, 0, P_ACCEPT, 0, u, v);
  return u < exp(-dH);
}

// ---- fused HMC trajectory ---------------------------------------------------------------------------
// Grid (nseg, B), NT threads, R consecutive sites per thread: buffer site k = t*R + r maps to global
// site (g0 + k) mod M.  halo == 0 means the buffer IS the periodic path (NT*R == M).  Otherwise the
// first / last `halo` = nt+1 buffer sites are recomputed copies of the neighbouring segments; the
// error front entering from the clamped buffer ends advances one site per leapfrog step and never
// reaches an owned site.  Only boundary values move through LDS (2 doubles per thread per step,
// double buffered -> one barrier per step).
//
// sampler/hmcsampler.cc:22-57: p ~ N(0,1); T0; nt+1 force evaluations with half steps for p at
// both ends and no position update after the last; T1; S(x_trial), S(x_cur).
template <int KIND, int R>
__global__ void __launch_bounds__(R >= 8 ? 512 : 1024)
    hmc_trajectory_kernel(PathP P, const double *__restrict__ x_cur, double *__restrict__ x_trial,
                          double *__restrict__ partials, const int32_t *__restrict__ done, uint32_t owned_len,
                          uint32_t halo, uint32_t nt, double dt, RngKey key0) {
  extern __shared__ double lds[];  // [2][2][NT] boundary exchange | 4*NT/64 reduction scratch | [R][NT] staging
  const uint32_t b = blockIdx.y, seg = blockIdx.x, t = threadIdx.x, NT = blockDim.x, M = P.M;
  if (done && done[b]) return;  // reference: repetitions after an acceptance are not run (hmcsampler.cc:10-12); null: none yet
  const bool periodic = (halo == 0);
  const uint32_t o0 = seg * owned_len;
  const uint32_t olen = min(owned_len, M - o0);
  const uint32_t g0 = (uint32_t)(((uint64_t)o0 + M - (halo % M)) % M);
  const uint32_t kbase = t * R;
  const double *xb = x_cur + (size_t)b * M;
  RngKey key = key0;
  key.chain += b;

  double *ex_first = lds, *ex_last = lds + 2 * NT;  // [2][NT] each
  double *stage = lds + 4 * NT + 4 * (NT / kWave);  // [R][NT]
  // Momenta are generated in a rolled loop through LDS: unrolled, the R Box-Muller chains get
  // interleaved and their temporaries push the 2R doubles of state out of the register file.
  {
    uint32_t g = (uint32_t)(((uint64_t)g0 + kbase) % M);
#pragma unroll 1
    for (int r = 0; r < R; ++r) {
      stage[r * NT + t] = rng_normal0(key, g, P_MOMENTUM, 0);
      g = (g + 1 == M) ? 0 : g + 1;
    }
  }
  double x[R], p[R];
  uint32_t g = (uint32_t)(((uint64_t)g0 + kbase) % M);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    x[r] = xb[g];
    p[r] = stage[r * NT + t];  // written by this thread: no barrier needed
    g = (g + 1 == M) ? 0 : g + 1;
  }

  int buf = 0;
  double xl, xr;
  auto exchange = [&]() {
    ex_first[buf * NT + t] = x[0];
    ex_last[buf * NT + t] = x[R - 1];
    __syncthreads();
    if (t == 0)
      xl = periodic ? ex_last[buf * NT + NT - 1] : x[0];
    else
      xl = ex_last[buf * NT + t - 1];
    if (t == NT - 1)
      xr = periodic ? ex_first[buf * NT] : x[R - 1];
    else
      xr = ex_first[buf * NT + t + 1];
    buf ^= 1;
  };

  // owned mask of buffer site k: halo <= k < halo + olen
  auto owned = [&](int r) { return (kbase + r - halo) < olen; };

  double sums[4] = {0.0, 0.0, 0.0, 0.0};  // S_cur, T0, S_trial, T1 (raw site sums)
  exchange();
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (owned(r)) {
      sums[0] += site_energy<KIND>(P, x[r], r == 0 ? xl : x[r - 1]);
      sums[1] += p[r] * p[r];
    }
    if (KIND == MLMCPI_ROTOR) __builtin_amdgcn_sched_barrier(0);
  }
  leapfrog<KIND, R>(P, x, p, xl, xr, nt, dt, exchange);

  double *xt = x_trial + (size_t)b * M;
  g = (uint32_t)(((uint64_t)g0 + kbase) % M);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (owned(r)) {
      sums[2] += site_energy<KIND>(P, x[r], r == 0 ? xl : x[r - 1]);
      sums[3] += p[r] * p[r];
      xt[g] = x[r];
    }
    g = (g + 1 == M) ? 0 : g + 1;
    if (KIND == MLMCPI_ROTOR) __builtin_amdgcn_sched_barrier(0);
  }
  block_sum<4>(sums, lds + 4 * NT);
  if (t == 0) {
    double *out = partials + ((size_t)b * gridDim.x + seg) * 4;
    out[0] = sums[0]; out[1] = sums[1]; out[2] = sums[2]; out[3] = sums[3];
  }
}

// Whole chains on the device: n_draws x n_rep trajectories of a periodic, register-resident path
// (one workgroup per chain) in ONE launch, with the Metropolis test, the copy-on-accept and the QoI
// of every draw done in-kernel.  Same arithmetic, same Philox counters (trajectory index
// traj0 + d*n_rep + r) as n_draws calls of mlmcpi_path_hmc_draw followed by the QoI kernel, so the
// two forms agree to rounding; this one removes ~2 launches and a host round trip per draw, which is
// what dominates for short paths (BASELINE config 1: M_lat = 128; the coarse levels of config 5).
// qoi_kind: 0 none, 1 <x^2> (qoixsquared.cc:7-20), 2 susceptibility (qoisusceptibility.cc:8-23).
template <int KIND, int R>
__global__ void __launch_bounds__(R >= 8 ? 512 : 1024)
    hmc_chain_kernel(PathP P, double *__restrict__ x_state, double *__restrict__ q_out,
                     int32_t *__restrict__ acc_count, double *__restrict__ energies, uint32_t nt, double dt,
                     uint32_t n_rep, uint32_t n_draws, int qoi_kind, RngKey key0) {
  extern __shared__ double lds[];  // [2][2][NT] exchange | 4*NT/64 scratch | [R][NT] staging | flag
  const uint32_t b = blockIdx.x, t = threadIdx.x, NT = blockDim.x, M = P.M;
  const uint32_t kbase = t * R;
  double *xb = x_state + (size_t)b * M;
  RngKey key = key0;
  key.chain += b;
  double *ex_first = lds, *ex_last = lds + 2 * NT;
  double *scratch = lds + 4 * NT;
  double *stage = scratch + 4 * (NT / kWave);
  double *flag = stage + (size_t)R * NT;
  const double escale = energy_scale(P);

  double xc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) xc[r] = xb[kbase + r];
  int buf = 0;
  // A chain that one wave holds (M = 64 R: BASELINE config 1, M_lat = 128) exchanges its boundary values by rotating the
  // wave one lane with DPP (wave_ror / wave_rol wrap around, which is the periodic boundary): four v_mov_b32_dpp instead
  // of two LDS writes, a barrier and two LDS reads per leapfrog step -- the step of such a chain is nothing but this latency.
  const bool one_wave = NT == kWave;
  auto exchange = [&](const double (&v)[R], double &xl, double &xr) {
    if (one_wave) {
      xl = wave_rotate_up(v[R - 1]);  // lane t gets lane t - 1 (lane 0: lane 63)
      xr = wave_rotate_down(v[0]);    // lane t gets lane t + 1 (lane 63: lane 0)
      return;
    }
    ex_first[buf * NT + t] = v[0];
    ex_last[buf * NT + t] = v[R - 1];
    __syncthreads();
    xl = ex_last[buf * NT + (t == 0 ? NT - 1 : t - 1)];
    xr = ex_first[buf * NT + (t == NT - 1 ? 0 : t + 1)];
    buf ^= 1;
  };
  int32_t n_acc = 0;
  for (uint32_t d = 0; d < n_draws; ++d) {
    bool accepted = false;
    for (uint32_t rep = 0; rep < n_rep && !accepted; ++rep) {
      key.step = key0.step + d * n_rep + rep;
      double x[R], p[R];
#pragma unroll 1
      for (int r = 0; r < R; ++r) stage[r * NT + t] = rng_normal0(key, kbase + r, P_MOMENTUM, 0);
#pragma unroll
      for (int r = 0; r < R; ++r) p[r] = stage[r * NT + t];
#pragma unroll
      for (int r = 0; r < R; ++r) x[r] = xc[r];
      double sums[4] = {0.0, 0.0, 0.0, 0.0};
      double xl, xr;
      exchange(x, xl, xr);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        sums[0] += site_energy<KIND>(P, x[r], r == 0 ? xl : x[r - 1]);
        sums[1] += p[r] * p[r];
        if (KIND == MLMCPI_ROTOR) __builtin_amdgcn_sched_barrier(0);
      }
      leapfrog<KIND, R>(P, x, p, xl, xr, nt, dt, [&]() { exchange(x, xl, xr); });
#pragma unroll
      for (int r = 0; r < R; ++r) {
        sums[2] += site_energy<KIND>(P, x[r], r == 0 ? xl : x[r - 1]);
        sums[3] += p[r] * p[r];
        if (KIND == MLMCPI_ROTOR) __builtin_amdgcn_sched_barrier(0);
      }
      block_sum<4>(sums, scratch);
      if (t == 0) flag[0] = hmc_decide(key, escale, sums, energies ? energies + 4 * (size_t)b : nullptr) ? 1.0 : 0.0;
      __syncthreads();
      accepted = flag[0] != 0.0;
      __syncthreads();  // flag is rewritten by the next repetition
      if (accepted) {
#pragma unroll
        for (int r = 0; r < R; ++r) xc[r] = x[r];
      }
    }
    n_acc += accepted ? 1 : 0;
    if (qoi_kind) {
      double q[1] = {0.0};
      if (qoi_kind == 1) {
#pragma unroll
        for (int r = 0; r < R; ++r) q[0] += xc[r] * xc[r];
      } else {
        double xl, xr;
        exchange(xc, xl, xr);
#pragma unroll
        for (int r = 0; r < R; ++r) q[0] += mod_2pi(xc[r] - (r == 0 ? xl : xc[r - 1]));
      }
      block_sum<1>(q, scratch);
      if (t == 0)
        q_out[(size_t)b * n_draws + d] =
            (qoi_kind == 1) ? (1.0 / M) * q[0] : (1. / (4. * kPi * kPi)) * (q[0] * q[0]) * (1.0 / P.T_final);
      __syncthreads();
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) xb[kbase + r] = xc[r];
  if (t == 0 && acc_count) acc_count[b] = n_acc;
}

// Global Metropolis test + copy of accepted trial states.  Grid (nblk, B).  Every workgroup of a
// chain recomputes the (cheap) decision from the segment partials in the same order, so no
// inter-workgroup hand-off is needed.  sampler/hmcsampler.cc:50-67.
__global__ void __launch_bounds__(256)
    hmc_accept_kernel(uint32_t M, double escale, double *__restrict__ x_cur, const double *__restrict__ x_trial,
                      const double *__restrict__ partials, uint32_t nseg, const int32_t *__restrict__ done_in,
                      int32_t *__restrict__ done_out, double *__restrict__ energies, RngKey key0) {
  const uint32_t b = blockIdx.y;
  if (done_in && done_in[b]) {  // (null: first repetition, no chain has accepted yet)
    if (blockIdx.x == 0 && threadIdx.x == 0) done_out[b] = 1;
    return;
  }
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (uint32_t k = 0; k < nseg; ++k) {
    const double *q = partials + ((size_t)b * nseg + k) * 4;
    s[0] += q[0]; s[1] += q[1]; s[2] += q[2]; s[3] += q[3];
  }
  RngKey key = key0;
  key.chain += b;
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  const bool acc = hmc_decide(key, escale, s, first && energies ? energies + 4 * (size_t)b : nullptr);
  if (first) done_out[b] = acc ? 1 : 0;
  if (!acc) return;
  double *dst = x_cur + (size_t)b * M;
  const double *src = x_trial + (size_t)b * M;
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < M; j += gridDim.x * blockDim.x) dst[j] = src[j];
}

__global__ void add_flags_kernel(int32_t *__restrict__ acc, const int32_t *__restrict__ flags, uint32_t B) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) acc[b] += flags[b];
}

struct HmcPlan {
  uint32_t R, NT, nseg, owned_len, halo;
};

// Register-resident geometry: the whole periodic path in one workgroup when M = NT*R fits
// (NT a multiple of 64, R in {1,2,4,8,16}, NT <= 512 for R >= 8 so that 2R doubles of state plus
// the sine's temporaries stay in VGPRs, else <= 1024), i.e. M <= 8192; longer paths are cut into
// segments of NT*R buffer sites with a halo of nt+1.
static int plan_hmc(int kind, uint32_t M, uint32_t B, uint32_t nt, HmcPlan *plan) {
  const uint32_t maxR = (kind == MLMCPI_ROTOR) ? 8 : 16;  // the rotor's sines need the registers
  static const uint32_t Rs[5] = {16, 8, 4, 2, 1};
  uint32_t best = 0, fallback = 0, best_nt = 0, fallback_nt = 0;
  for (uint32_t R : Rs) {
    if (R > maxR || M % R) continue;
    uint32_t NT = M / R;
    if (NT % 64 || NT < 64 || NT > (R >= 8 ? 512u : 1024u)) continue;  // register budget: see launch bounds
    if (!fallback || NT > fallback_nt) { fallback = R; fallback_nt = NT; }  // most parallel
    if (!best && (uint64_t)B * (NT / 64) >= 2048) { best = R; best_nt = NT; }  // largest R that still fills the chip
  }
  if (best || fallback) {
    plan->R = best ? best : fallback;
    plan->NT = best ? best_nt : fallback_nt;
    plan->nseg = 1;
    plan->owned_len = M;
    plan->halo = 0;
    return MLMCPI_OK;
  }
  const uint32_t halo = nt + 1;
  uint32_t R = maxR, NT = 4096 / maxR;
  if (M + 2 * halo <= 1024) { R = 4; NT = 256; }  // short odd-sized paths
  const uint32_t L = NT * R;
  if (2 * halo + 64 > L) return fail(MLMCPI_ERR_INVALID, "nt = %u too long for the fused trajectory (max %u)", nt, (L - 64) / 2 - 1);
  const uint32_t owned_max = L - 2 * halo;
  const uint32_t nseg = (M + owned_max - 1) / owned_max;
  plan->R = R;
  plan->NT = NT;
  plan->nseg = nseg;
  plan->owned_len = (M + nseg - 1) / nseg;
  plan->halo = halo;
  return MLMCPI_OK;
}

// f(std::integral_constant<int, R>{}) for the plan's sites per thread
template <class F>
static void dispatch_R(uint32_t R, F &&f) {
  switch (R) {
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 1>{});
  }
}

template <int KIND>
static int launch_traj(const HmcPlan &pl, const PathP &P, const double *x_cur, double *x_trial, double *partials,
                       const int32_t *done, uint32_t B, uint32_t nt, double dt, RngKey key, hipStream_t st) {
  dim3 grid(pl.nseg, B), block(pl.NT);
  const size_t lds = (4 * pl.NT + 4 * (pl.NT / 64) + (size_t)pl.R * pl.NT) * sizeof(double);
  dispatch_R(pl.R, [&](auto R) {
    hipLaunchKernelGGL((hmc_trajectory_kernel<KIND, decltype(R)::value>), grid, block, lds, st, P, x_cur, x_trial, partials, done,
                       pl.owned_len, pl.halo, nt, dt, key);
  });
  MLMCPI_LAUNCH_CHECK("hmc_trajectory_kernel");
  return MLMCPI_OK;
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

// workspace layout: x_trial [B*M] | partials [B*nseg*4] | flags [2][B] int32
int mlmcpi_path_hmc_workspace_bytes(const mlmcpi_path_action *act, uint32_t B, uint32_t nt, size_t *bytes) {
  if (int rc = check_action(act)) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  HmcPlan pl;
  if (int rc = plan_hmc(act->kind, act->M, B, nt, &pl)) return rc;
  *bytes = align256((size_t)B * act->M * 8) + align256((size_t)B * pl.nseg * 4 * 8) + align256((size_t)2 * B * 4);
  return MLMCPI_OK;
}

int mlmcpi_path_hmc_draw(const mlmcpi_path_action *act, double *d_x, uint32_t B, uint32_t nt, double dt,
                         uint32_t n_rep, uint64_t seed, uint32_t chain0, uint32_t traj0, void *d_work,
                         int32_t *d_accept, double *d_energies, void *stream) {
  if (int rc = check_action(act)) return rc;
  MLMCPI_REQUIRE(d_x && d_work && B > 0 && n_rep > 0, "bad arguments");
  HmcPlan pl;
  if (int rc = plan_hmc(act->kind, act->M, B, nt, &pl)) return rc;
  PathP P = make_params(*act);
  hipStream_t st = as_stream(stream);
  char *w = (char *)d_work;
  double *x_trial = (double *)w;
  w += align256((size_t)B * P.M * 8);
  double *partials = (double *)w;
  w += align256((size_t)B * pl.nseg * 4 * 8);
  int32_t *flags = (int32_t *)w;  // [2][B]
  // accept flags ping-pong between the two halves of `flags`; the first repetition has none to read (null) and the last
  // one writes the caller's array directly: a draw is n_rep x (trajectory, accept) and nothing else on the stream
  const uint32_t copy_blocks = choose_split(P.M, B);
  for (uint32_t r = 0; r < n_rep; ++r) {
    const int32_t *done_in = r == 0 ? nullptr : flags + (size_t)(r & 1) * B;
    int32_t *done_out = (r + 1 == n_rep && d_accept) ? d_accept : flags + (size_t)((r + 1) & 1) * B;
    RngKey key = make_key(seed, chain0, traj0 + r);
    const int rc = dispatch_kind(P.kind, [&](auto K) {
      return launch_traj<decltype(K)::value>(pl, P, d_x, x_trial, partials, done_in, B, nt, dt, key, st);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(hmc_accept_kernel, dim3(copy_blocks, B), dim3(256), 0, st, P.M, energy_scale(P), d_x,
                       (const double *)x_trial, (const double *)partials, pl.nseg, done_in, done_out, d_energies, key);
    MLMCPI_LAUNCH_CHECK("hmc_accept_kernel");
  }
  return MLMCPI_OK;
}

int mlmcpi_path_hmc_run(const mlmcpi_path_action *act, double *d_x, uint32_t B, uint32_t nt, double dt, uint32_t n_rep,
                        uint32_t n_draws, int qoi_kind, uint64_t seed, uint32_t chain0, uint32_t traj0, void *d_work,
                        double *d_qoi, int32_t *d_accept_count, void *stream) {
  if (int rc = check_action(act)) return rc;
  MLMCPI_REQUIRE(d_x && d_work && B > 0 && n_rep > 0 && n_draws > 0, "bad arguments");
  MLMCPI_REQUIRE(qoi_kind >= 0 && qoi_kind <= 2 && (qoi_kind == 0 || d_qoi), "bad QoI selection");
  HmcPlan pl;
  if (int rc = plan_hmc(act->kind, act->M, B, nt, &pl)) return rc;
  PathP P = make_params(*act);
  hipStream_t st = as_stream(stream);
  if (pl.halo == 0) {
    // register-resident periodic path: everything in one launch, one workgroup per chain
    const size_t lds = (4 * pl.NT + 4 * (pl.NT / 64) + (size_t)pl.R * pl.NT + 1) * sizeof(double);
    const RngKey key = make_key(seed, chain0, traj0);
    dispatch_kind(P.kind, [&](auto K) {
      dispatch_R(pl.R, [&](auto R) {
        hipLaunchKernelGGL((hmc_chain_kernel<decltype(K)::value, decltype(R)::value>), dim3(B), dim3(pl.NT), lds, st, P, d_x, d_qoi,
                           d_accept_count, (double *)nullptr, nt, dt, n_rep, n_draws, qoi_kind, key);
      });
    });
    MLMCPI_LAUNCH_CHECK("hmc_chain_kernel");
    return MLMCPI_OK;
  }
  // segmented paths (M > 8192 or not a multiple of 64): same sequence through the per-draw entry points
  int32_t *acc_tmp = nullptr;
  if (d_accept_count) MLMCPI_HIP_TRY(hipMemsetAsync(d_accept_count, 0, (size_t)B * 4, st));
  MLMCPI_HIP_TRY(hipMalloc((void **)&acc_tmp, (size_t)B * 4));
  int rc = MLMCPI_OK;
  for (uint32_t d = 0; d < n_draws && !rc; ++d) {
    rc = mlmcpi_path_hmc_draw(act, d_x, B, nt, dt, n_rep, seed, chain0, traj0 + d * n_rep, d_work, acc_tmp, nullptr, stream);
    if (!rc && d_accept_count) {
      hipLaunchKernelGGL(add_flags_kernel, dim3((B + 255) / 256), dim3(256), 0, st, d_accept_count, (const int32_t *)acc_tmp, B);
    }
    if (!rc && qoi_kind == 1) rc = path_reduce(R_XSQUARED, P, d_x, B, 1.0 / P.M, d_qoi + (size_t)d * B, st);
    if (!rc && qoi_kind == 2) rc = path_reduce(R_WINDING, P, d_x, B, 1.0 / P.T_final, d_qoi + (size_t)d * B, st);
  }
  (void)hipStreamSynchronize(st);
  (void)hipFree(acc_tmp);
  return rc;
}

int mlmcpi_path_hmc_run_layout(const mlmcpi_path_action *act, uint32_t B, uint32_t nt, int32_t *chain_major) {
  if (int rc = check_action(act)) return rc;
  MLMCPI_REQUIRE(chain_major && B > 0, "bad arguments");
  HmcPlan pl;
  if (int rc = plan_hmc(act->kind, act->M, B, nt, &pl)) return rc;
  *chain_major = pl.halo == 0 ? 1 : 0;
  return MLMCPI_OK;
}

// host only: the plan the three entry points above run, and plan_hmc's own status for an nt that is too long
int mlmcpi_path_hmc_plan(const mlmcpi_path_action *act, uint32_t B, uint32_t nt, mlmcpi_path_hmc_plan_info *out) {
  if (int rc = check_action(act)) return rc;
  MLMCPI_REQUIRE(out && B > 0, "bad arguments");
  HmcPlan pl;
  if (int rc = plan_hmc(act->kind, act->M, B, nt, &pl)) return rc;
  out->R = pl.R;
  out->NT = pl.NT;
  out->nseg = pl.nseg;
  out->owned_len = pl.owned_len;
  out->halo = pl.halo;
  out->chain_major = pl.halo == 0 ? 1 : 0;
  return MLMCPI_OK;
}

}  // extern "C"
