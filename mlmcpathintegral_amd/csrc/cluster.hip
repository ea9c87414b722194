// cluster.hip -- the cluster samplers (gfx950, wave64).
//
//   ClusterSampler::draw, 1-D (single_cluster_update1d)        sampler/clustersampler.cc:36-49, 92-132
//     with RotorAction::{new_reflection, S_ell, flip}          action/qm/rotoraction.hh:226-253
//   QuenchedSchwingerClusterSampler::draw                      sampler/quenchedschwingerclustersampler.cc:40-86
//
// The rotor update, restated.  With xbar the reflection angle and c_j = cos(x_j - xbar) of the path BEFORE
// the update, the link l = (l, l + 1 mod M) is bonded with probability  p_l = 1 - exp(min(0, -(2 m0 / a) c_l c_{l+1}))  --
// symmetric, and a function of the starting path only (flipping a site negates its c, which is what the reference's walk
// sees when it evaluates S_ell from an already flipped site).  One update = M independent Bernoulli bonds; the cluster is
// the run of bonded links that contains the seed site i0; every site of it is reflected, x <- mod_2pi(pi + 2 xbar - x).
// Every uniform is a pure function of (link, chain, update counter), so the bonds need only be looked at in a window around
// i0 that grows until an open link is found on each side.  If the run reaches all M sites, all M are flipped once.
//
// RNG contract:
//   P_CLUSTER_REFLECT  site 0, step = global update counter:  xbar = 2 pi u - pi,  i0 = min(floor(v M), M - 1)
//   P_CLUSTER_BOND     site l >> 1, same step:  u decides link l even, v link l odd;  bonded iff uniform < p_l
//   P_GAUGE            site vertex >> 1 (vertex = Mt j + i), step = draw counter:  g = 2 pi (u | v by parity) - pi
#include "internal.hpp"

namespace mlmcpi {

constexpr int kClusterWaves = 4;   // waves per workgroup (one chain / column group each; no LDS, no barriers)
constexpr int kWindow = 63;        // links a wave looks at per round: 64 sites, 63 links between them

__device__ __forceinline__ double bond_uniform(const RngKey &key, uint32_t link) {
  const U4 r = philox4x32_10(link >> 1, key.chain, key.step, (uint32_t)P_CLUSTER_BOND << 24, key.k0, key.k1);
  return (link & 1u) ? u01(r.z, r.w) : u01(r.x, r.y);
}

// One direction of one update.  Lane k of round r holds the site at distance o = 63 r + k from the seed (DIR = +1: i0 + o,
// -1: i0 - o) and, for k < 63, the link towards distance o + 1.  Links at distance >= lim count as open, so the scan ends
// there at the latest.  Sites up to the first open link are reflected in place (distance 0 only when DIR > 0: the seed is
// flipped once, and the backward scan takes its cosine, c0, from before the flip).  Returns the number of bonded links.
template <int DIR>
__device__ __forceinline__ uint32_t cluster_scan(double *x, uint32_t M, uint32_t i0, uint32_t lim, double xbar, double kappa2,
                                                 const RngKey &key, uint32_t lane, double &c0) {
  uint32_t base = 0;
  for (;;) {
    const uint32_t o = base + lane;
    const bool site_ok = o <= lim;                       // lim <= M - 1: the sites of a scan are distinct
    // in [0, 2 M) wherever site_ok (i0 < M, o <= M - 1).  Lanes beyond lim (o may exceed i0 + M: the unsigned difference
    // wraps) get a meaningless s and link; neither is used: no load, no bond test, no store for them.
    uint32_t s = DIR > 0 ? i0 + o : i0 + M - o;
    if (s >= M) s -= M;
    const bool seed_again = DIR < 0 && o == 0;
    double xv = 0.0;
    if (site_ok && !seed_again) xv = x[s];
    double c = cos(xv - xbar);
    if (DIR > 0 && base == 0) c0 = __shfl(c, 0);
    if (seed_again) c = c0;
    const double cn = __shfl_down(c, 1);
    const uint32_t link = DIR > 0 ? s : (s == 0 ? M - 1 : s - 1);
    bool bonded = false;
    if (lane < (uint32_t)kWindow && o < lim) {
      const double p = 1.0 - exp(fmin(0.0, -(kappa2 * c) * cn));
      bonded = bond_uniform(key, link) < p;
    }
    const unsigned long long open = ~__ballot(bonded);   // lane 63 is never bonded: open != 0
    const uint32_t j = (uint32_t)__builtin_ctzll(open);
    if (lane <= j && lane < (uint32_t)kWindow && !seed_again) x[s] = mod_2pi(kPi + 2.0 * xbar - xv);
    if (j < (uint32_t)kWindow) return base + j;
    base += kWindow;                                     // all 63 bonded: lane 63's site is lane 0 of the next round
  }
}

// n_updates reflection-cluster updates of B chains, in place; one wave per chain.
__global__ void __launch_bounds__(kClusterWaves * kWave)
    rotor_cluster_kernel(double *x_all, uint32_t M, double kappa2, uint32_t B, uint32_t n_updates, RngKey key0,
                         uint32_t *cluster_sites) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t b = blockIdx.x * kClusterWaves + (threadIdx.x >> 6);
  if (b >= B) return;                                    // wave uniform
  double *x = x_all + (size_t)b * M;
  RngKey key = key0;
  key.chain = key0.chain + b;
  uint32_t total = 0;
  for (uint32_t n = 0; n < n_updates; ++n, ++key.step) {
    double u, v;
    rng_uniforms(key, 0, P_CLUSTER_REFLECT, 0, u, v);
    const double xbar = fma(kTwoPi, u, -kPi);
    uint32_t i0 = (uint32_t)(v * (double)M);
    i0 = __builtin_amdgcn_readfirstlane(i0 < M ? i0 : M - 1);
    double c0 = 0.0;
    const uint32_t f = cluster_scan<+1>(x, M, i0, M - 1, xbar, kappa2, key, lane, c0);
    uint32_t back = 0;
    if (f < M - 1) back = cluster_scan<-1>(x, M, i0, M - 1 - f, xbar, kappa2, key, lane, c0);
    total += f + back + 1;
    // the next update of this chain reads what this one stored (same wave, other lanes): drain the stores first
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  }
  if (cluster_sites && lane == 0) cluster_sites[b] += total;
}

// ---- quenched Schwinger: links from the plaquette path ---------------------------------------------------------------
// psi[c], c = i Mx + j, is a closed path of N = Mt Mx angles; d[c] = psi[c + 1] - psi[c].  The reference's sequential
// construction in closed form:
//   theta_1(i, j) = sum_{i' < i} d[i' Mx + j]                                        (prefix sum up column j)
//   theta_0(i, j) = 0 for i < Mt - 1;  theta_0(Mt - 1, j) = -sum_{j' < j} sum_{i'} d[i' Mx + j']
//                 = -sum_{i'} (psi[i' Mx + j] - psi[i' Mx])                          (the sum over j' telescopes)
//   then theta_0(i, j) += g(i, j) - g(i + 1, j),  theta_1(i, j) += g(i, j) - g(i, j + 1)  (periodic), mod_2pi.
// theta[2 Mt j + 2 i + mu] has i fastest, psi has j fastest.  The stores (16 B per vertex) are the larger stream, so lanes
// run along i: a wave owns kCols = 8 adjacent columns of one chain and walks up the rows 64 at a time, lane = row.  Each
// lane reads the 9 consecutive psi of its row (a 64-B line serves 8 columns: the first load of a round brings the lines in,
// the others hit L1), the prefix over rows is a wave scan plus a carry, the gauge angles cost one Philox call per vertex, and a lane's (theta_0, theta_1) pairs go out as
// 1-KiB coalesced non-temporal stores per column.  No LDS, no barrier, one launch.
constexpr int kCols = 8;

__device__ __forceinline__ double gauge_angle(const RngKey &key, uint32_t vertex) {
  const U4 r = philox4x32_10(vertex >> 1, key.chain, key.step, (uint32_t)P_GAUGE << 24, key.k0, key.k1);
  return fma(kTwoPi, (vertex & 1u) ? u01(r.z, r.w) : u01(r.x, r.y), -kPi);
}

typedef double cl_d2_t __attribute__((ext_vector_type(2)));

__global__ void __launch_bounds__(kClusterWaves * kWave)
    schwinger_cluster_links_kernel(const double *__restrict__ psi_all, double *__restrict__ theta_all, uint32_t Mt, uint32_t Mx,
                                   uint32_t B, uint32_t groups, int gauge, RngKey key0) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t w = blockIdx.x * kClusterWaves + (threadIdx.x >> 6);
  if (w >= B * groups) return;                           // wave uniform
  const uint32_t b = w / groups, j0 = (w - b * groups) * kCols;
  const size_t N = (size_t)Mt * Mx;
  const double *psi = psi_all + (size_t)b * N;
  double *theta = theta_all + (size_t)b * 2 * N;
  RngKey key = key0;
  key.chain = key0.chain + b;
  double carry[kCols], colsum[kCols];  // prefix of d over the rows below this round; per-lane sums of psi[i, j] - psi[i, 0]
#pragma unroll
  for (int q = 0; q < kCols; ++q) carry[q] = colsum[q] = 0.0;
  // Gauge angles: ONE Philox call per vertex and wave.  gc[q] = g(i, j0 + q) of this round's rows for the 8 columns and the
  // column behind them (g(i, j + 1) of column q is gc[q + 1]); g(i + 1, j) is the next lane's gc[q], for lane 63 lane 0 of
  // the next round's angles gn[q] (drawn one round ahead), for the top row g(0, j) = g0[q], kept from the first round.
  double gc[kCols + 1], gn[kCols + 1], g0[kCols + 1];
  uint32_t vcol[kCols + 1];            // Mt * column, the column behind the last wraps to 0 (ragged groups: unused values)
#pragma unroll
  for (int q = 0; q <= kCols; ++q) {
    const uint32_t j = j0 + q;
    vcol[q] = Mt * (j < Mx ? j : j - Mx);
    gc[q] = gn[q] = g0[q] = 0.0;
    if (gauge) {
      gc[q] = gauge_angle(key, vcol[q] + (lane < Mt ? lane : Mt - 1));
      g0[q] = __shfl(gc[q], 0);
    }
  }

  for (uint32_t i_base = 0; i_base < Mt; i_base += kWave) {
    const uint32_t i = i_base + lane;
    const bool row_ok = i < Mt;
    const bool last_round = i_base + kWave >= Mt;        // wave uniform
    double p[kCols + 1], p0 = 0.0;
#pragma unroll
    for (int q = 0; q <= kCols; ++q) {
      const size_t idx = (size_t)i * Mx + j0 + q;        // psi[N] (behind the last cell) is never used: reads as 0
      p[q] = (row_ok && idx < N) ? psi[idx] : 0.0;
    }
    if (row_ok) p0 = psi[(size_t)i * Mx];
    if (gauge && !last_round) {                          // wave uniform
      const uint32_t in = i + kWave;
#pragma unroll
      for (int q = 0; q <= kCols; ++q) gn[q] = gauge_angle(key, vcol[q] + (in < Mt ? in : Mt - 1));
    }
#pragma unroll
    for (int q = 0; q < kCols; ++q) {
      const uint32_t j = j0 + q;
      const bool ok = row_ok && j < Mx;
      double inc = ok ? p[q + 1] - p[q] : 0.0;           // inclusive scan over the rows of this round
#pragma unroll
      for (int d = 1; d < kWave; d <<= 1) {
        const double t = __shfl_up(inc, d);
        if (lane >= (uint32_t)d) inc += t;
      }
      const double below = __shfl_up(inc, 1);
      double t1 = carry[q] + (lane ? below : 0.0), t0 = 0.0;
      carry[q] += __shfl(inc, kWave - 1);
      if (ok) colsum[q] += p[q] - p0;
      if (last_round) {
        const double total = __shfl(wave_sum(colsum[q]), 0);
        if (i + 1 == Mt) t0 = -total;
      }
      if (gauge) {                                       // wave uniform: the shuffles run with every lane
        const double next_lane = __shfl_down(gc[q], 1), next_round = __shfl(gn[q], 0);
        const double g_up = i + 1 == Mt ? g0[q] : (lane == kWave - 1 ? next_round : next_lane);
        t0 += gc[q] - g_up;
        t1 += gc[q] - gc[q + 1];
      }
      if (ok) {
        cl_d2_t v;
        v.x = mod_2pi(t0);
        v.y = mod_2pi(t1);
        __builtin_nontemporal_store(v, reinterpret_cast<cl_d2_t *>(theta + 2 * ((size_t)Mt * j + i)));
      }
    }
#pragma unroll
    for (int q = 0; q <= kCols; ++q) gc[q] = gn[q];
  }
}

static int check_rotor(const mlmcpi_path_action *act, const char *what) {
  if (!act) return fail(MLMCPI_ERR_INVALID, "action is NULL");
  if (act->kind != MLMCPI_ROTOR)
    return fail(MLMCPI_ERR_UNSUPPORTED,
                "%s: the 1-D cluster sampler is defined for the rotor only (harmonic / quartic oscillator: no reflection "
                "symmetry of the bond form); action kind %d", what, act->kind);
  if (act->M < 2 || act->M > (1u << 30)) return fail(MLMCPI_ERR_INVALID, "M_lat = %u out of range", act->M);
  if (!(act->T_final > 0.0) || !(act->m0 > 0.0)) return fail(MLMCPI_ERR_INVALID, "T_final and m0 must be positive");
  return MLMCPI_OK;
}

static int check_schwinger(const mlmcpi_lattice_action *act, const char *what) {
  if (!act) return fail(MLMCPI_ERR_INVALID, "action is NULL");
  if (act->kind == MLMCPI_NONLINEAR_SIGMA)
    return fail(MLMCPI_ERR_UNSUPPORTED, "%s: the generic 2-D cluster update of the sigma model (connected components on the "
                "lattice) is not implemented (DESIGN.md 8)", what);
  if (act->kind != MLMCPI_SCHWINGER)
    return fail(MLMCPI_ERR_UNSUPPORTED, "%s: cluster not supported for chosen action (kind %d)", what, act->kind);
  if (act->Mt < 2 || act->Mx < 2 || (uint64_t)act->Mt * act->Mx > (1u << 30))
    return fail(MLMCPI_ERR_INVALID, "lattice %u x %u out of range", act->Mt, act->Mx);
  if (!(act->beta > 0.0)) return fail(MLMCPI_ERR_INVALID, "beta must be positive");
  return MLMCPI_OK;
}

static int launch_rotor_cluster(double *d_x, uint32_t M, double kappa2, uint32_t B, uint32_t n_updates, uint64_t seed,
                                uint32_t chain0, uint32_t update0, uint32_t *d_cluster_sites, hipStream_t st) {
  const uint32_t blocks = (B + kClusterWaves - 1) / kClusterWaves;
  hipLaunchKernelGGL(rotor_cluster_kernel, dim3(blocks), dim3(kClusterWaves * kWave), 0, st, d_x, M, kappa2, B, n_updates,
                     make_key(seed, chain0, update0), d_cluster_sites);
  MLMCPI_LAUNCH_CHECK("rotor_cluster_kernel");
  return MLMCPI_OK;
}

static int launch_links(const mlmcpi_lattice_action *act, const double *d_psi, double *d_theta, uint32_t B, int gauge,
                        uint64_t seed, uint32_t chain0, uint32_t draw0, hipStream_t st) {
  const uint32_t groups = (act->Mx + kCols - 1) / kCols;
  const uint64_t waves = (uint64_t)B * groups;
  MLMCPI_REQUIRE(waves <= 0x7FFFFFFFull, "batch too large");
  const uint32_t blocks = (uint32_t)((waves + kClusterWaves - 1) / kClusterWaves);
  hipLaunchKernelGGL(schwinger_cluster_links_kernel, dim3(blocks), dim3(kClusterWaves * kWave), 0, st, d_psi, d_theta, act->Mt,
                     act->Mx, B, groups, gauge, make_key(seed, chain0, draw0));
  MLMCPI_LAUNCH_CHECK("schwinger_cluster_links_kernel");
  return MLMCPI_OK;
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_path_cluster_draw(const mlmcpi_path_action *act, double *d_x, uint32_t B, uint32_t n_updates, uint64_t seed,
                             uint32_t chain0, uint32_t update0, uint32_t *d_cluster_sites, void *stream) {
  if (int rc = check_rotor(act, "mlmcpi_path_cluster_draw")) return rc;
  MLMCPI_REQUIRE(d_x && B > 0, "bad arguments");
  MLMCPI_REQUIRE((uint64_t)update0 + n_updates <= 0xFFFFFFFFull, "update counter overflows");
  const double a = act->T_final / act->M;
  return launch_rotor_cluster(d_x, act->M, 2.0 * act->m0 / a, B, n_updates, seed, chain0, update0, d_cluster_sites,
                              as_stream(stream));
}

int mlmcpi_schwinger_cluster_workspace_bytes(const mlmcpi_lattice_action *act, uint32_t B, size_t *bytes) {
  if (int rc = check_schwinger(act, "mlmcpi_schwinger_cluster_workspace_bytes")) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  *bytes = align256((size_t)B * sizeof(uint32_t));  // flipped sites per chain, added up over the draws (zeroed by the caller)
  return MLMCPI_OK;
}

int mlmcpi_schwinger_cluster_init(const mlmcpi_lattice_action *act, double *d_psi, uint32_t B, uint64_t seed, uint32_t chain0,
                                  void *stream) {
  if (int rc = check_schwinger(act, "mlmcpi_schwinger_cluster_init")) return rc;
  // quenchedschwingerclustersampler.cc:19-26: a rotor on Lattice1D(N, 1.0) with m0 = beta a; RotorAction::initialise_state
  const uint32_t N = act->Mt * act->Mx;
  const mlmcpi_path_action rotor = {MLMCPI_ROTOR, N, 1.0, act->beta / N, 0.0, 0.0, 0.0};
  return mlmcpi_path_initialise(&rotor, d_psi, B, seed, chain0, stream);
}

int mlmcpi_schwinger_cluster_links(const mlmcpi_lattice_action *act, const double *d_psi, double *d_theta, uint32_t B, int gauge,
                                   uint64_t seed, uint32_t chain0, uint32_t draw0, void *stream) {
  if (int rc = check_schwinger(act, "mlmcpi_schwinger_cluster_links")) return rc;
  MLMCPI_REQUIRE(d_psi && d_theta && B > 0, "bad arguments");
  return launch_links(act, d_psi, d_theta, B, gauge, seed, chain0, draw0, as_stream(stream));
}

int mlmcpi_schwinger_cluster_draw(const mlmcpi_lattice_action *act, double *d_psi, double *d_theta, uint32_t B,
                                  uint32_t n_updates, uint64_t seed, uint32_t chain0, uint32_t draw0, double *d_work,
                                  void *stream) {
  if (int rc = check_schwinger(act, "mlmcpi_schwinger_cluster_draw")) return rc;
  MLMCPI_REQUIRE(d_psi && d_theta && d_work && B > 0, "bad arguments");
  MLMCPI_REQUIRE((uint64_t)draw0 * n_updates + n_updates <= 0xFFFFFFFFull, "update counter overflows");
  // m0 / a = beta, so 2 m0 / a = 2 beta.  Update k of draw d has the counter d n_updates + k.
  if (int rc = launch_rotor_cluster(d_psi, act->Mt * act->Mx, 2.0 * act->beta, B, n_updates, seed, chain0, draw0 * n_updates,
                                    (uint32_t *)d_work, as_stream(stream)))
    return rc;
  return launch_links(act, d_psi, d_theta, B, 1, seed, chain0, draw0, as_stream(stream));
}

}  // extern "C"
