// sigma_level_cluster.hip -- the Wolff single-cluster update of the O(3) nonlinear sigma model on the levels of its
// CoarsenRotate hierarchy (include/mlmcpi_hip.h: mlmcpi_sigma_level_cluster_*).  An unrotated level is the
// lattice of sigma_cluster.hip and delegates to mlmcpi_sigma_cluster_*; this file adds the ROTATED level (geometry:
// sigma_level_device.hpp), where the coarse sampler of a two-level or hierarchical run with two levels lives.
//
// The update, restated (tests/sigma_level_cluster_model.py).  The level has n = Mt Mx / 2 vertices, plane E then plane O of
// ht x hx = Mt/2 x Mx/2 each.  It is bipartite: every link has exactly one E end, so the 2 n links are named (e, d) with e an E
// vertex (e < n / 2) and d its direction in the reference's order: E(a, b) -> O(a, b), O(a, b-1), O(a-1, b), O(a-1, b-1).  Seen from
// O(a, b), direction d' -> E(a+1, b+1), E(a+1, b), E(a, b+1), E(a, b) crosses link (neighbour, 3 - d').  Where a plane extent is
// 1 several of the four neighbours of a vertex are one vertex; those are distinct links with a uniform each, as the action
// counts each of those bonds (the rule of the unrotated kernel at an extent of 2).  With r the reflection normal and a_l = r .
// sigma_l of the field BEFORE the update, link (x, y) is bonded iff (a_x a_y) > 0 and its uniform < 1 - exp(min(0, -2 beta
// (a_x a_y))); the cluster is the connected component of the seed vertex in the graph of bonded links; every vertex of it is
// reflected once, sigma' = sigma - 2 a r, and stored in the canonical form.  Every decision is a function of (link, chain,
// update counter, field before the update): the result does not depend on the order of the traversal.
//
// RNG contract, step = global update counter, the purposes of the unrotated update with the level's indices:
//   P_SIGMA_REFLECT  site 0, sub 0: (u, v) -> r_z = 1 - 2 u, azimuth 2 pi v - pi;  sub 1: u -> seed vertex min(floor(u n), n - 1)
//   P_SIGMA_BOND     site e, sub d >> 1: u decides link (e, d) for d even, v for d odd
#include <mutex>

#include "internal.hpp"

#include "sigma_device.hpp"  // fp contraction is off from here on
#include "sigma_level_device.hpp"

namespace mlmcpi {

// the launch plan's constants are those of sigma_cluster.hip, applied to n
constexpr uint32_t kSlcWaveChains = 4;          // team = wave: chains per workgroup of 256 threads
constexpr uint32_t kSlcWaveLdsWords = 2048;     // team = wave: bitmap in LDS up to 8 KiB per chain (65 536 vertices)
constexpr uint32_t kSlcBlockLdsWords = 32768;   // team = workgroup: bitmap in LDS up to 128 KiB (2^20 vertices)
constexpr uint32_t kSlcBlockThreads = 1024;

// What orders one phase of a team behind the one before it: the phase's stores (state, queue, bitmap) drained and, for a
// team of several waves, the barrier.  A team of one wave runs in lockstep and needs the drain only.
template <bool BLOCK>
__device__ __forceinline__ void slc_team_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  if (BLOCK) __syncthreads();
  else __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double slc_reflect_dot(const V3 &r, const V3 &s) { return (r.x * s.x + r.y * s.y) + r.z * s.z; }

// n_updates updates of every chain of a rotated level, in place: the algorithm of sigma_cluster_kernel (teams of one wave or
// one workgroup; frontier expansion over a queue of (vertex, a) pairs; a lane takes one (frontier vertex, direction) task,
// pre-checks the membership bitmap with a relaxed atomic load and claims the neighbour with an atomic OR; one ballot, one
// prefix count and one atomic add on the tail counter per wave and round; reflections from the queue once growth has ended,
// the same pass clearing the members' bitmap words) with the neighbour and the link of a task from the plane arithmetic
// above.  The queue carries the linear index: one division by ht per task (DESIGN.md 4.6a says why not (a, b, p) packed).
// The frontier loop ends after at most n levels (a vertex joins once, a level without a new member is the last one); `level <
// n` states that cap explicitly.  Queue positions are < n for the same reason; the store is guarded all the same.
template <bool BLOCK, bool LDS_MAP>
__global__ void __launch_bounds__(BLOCK ? kSlcBlockThreads : kSlcWaveChains * kWave)
    sigma_rot_cluster_kernel(double2 *phi_all, SigmaLevel L, double beta2, uint32_t B, uint32_t n_updates, RngKey key0,
                             uint32_t *queue_vertex, double *queue_a, uint32_t *map_all, uint32_t words, uint32_t *cluster_sites) {
  extern __shared__ uint32_t lds_map[];
  __shared__ uint32_t s_tail[kSlcWaveChains];
  const uint32_t T = BLOCK ? blockDim.x : (uint32_t)kWave;
  const uint32_t lane = BLOCK ? threadIdx.x : threadIdx.x & (kWave - 1);
  const uint32_t wave_lane = threadIdx.x & (kWave - 1);
  const uint32_t slot = BLOCK ? 0 : threadIdx.x >> 6;
  const uint32_t b = BLOCK ? blockIdx.x : blockIdx.x * kSlcWaveChains + slot;
  if (b >= B) return;                                    // team uniform (BLOCK: the grid has B workgroups)
  const uint32_t n = L.nvert(), ht = L.ht, hx = L.hx, nq = L.q;
  double2 *phi = phi_all + (size_t)b * n;
  uint32_t *qv = queue_vertex + (size_t)b * n;
  double *qa = queue_a + (size_t)b * n;
  uint32_t *map = LDS_MAP ? lds_map + slot * words : map_all + (size_t)b * words;
  for (uint32_t w = lane; w < words; w += T) map[w] = 0;
  RngKey key = key0;
  key.chain = key0.chain + b;
  uint32_t total = 0;
  slc_team_sync<BLOCK>();

  for (uint32_t k = 0; k < n_updates; ++k, ++key.step) {
    double u, v, us, unused;
    rng_uniforms(key, 0, P_SIGMA_REFLECT, 0, u, v);
    rng_uniforms(key, 0, P_SIGMA_REFLECT, 1, us, unused);
    const double rz = 1.0 - 2.0 * u, t = 1.0 - rz * rz, rho = t > 0.0 ? sqrt(t) : 0.0;
    double sa, ca;
    sincos(kTwoPi * v - kPi, &sa, &ca);
    const V3 r{rho * ca, rho * sa, rz};
    uint32_t seed = (uint32_t)(us * (double)n);
    seed = seed < n ? seed : n - 1;
    if (lane == 0) {
      qv[0] = seed;
      qa[0] = slc_reflect_dot(r, sigma_of(phi[seed]));
      map[seed >> 5] = 1u << (seed & 31u);
      s_tail[slot] = 1;
    }
    slc_team_sync<BLOCK>();

    uint32_t head = 0, tail = 1;
    for (uint32_t level = 0; level < n && head < tail; ++level) {
      for (uint32_t base = head; base < tail; base += T / 4) {  // team uniform trip count: the ballot below sees whole waves
        const uint32_t q = base + (lane >> 2), d = lane & 3u;
        bool add = false;
        uint32_t y = 0;
        double ay = 0.0;
        if (q < tail) {
          const uint32_t x = qv[q];
          const double ax = qa[q];
          const bool odd = x >= nq;                      // plane O
          const uint32_t c = odd ? x - nq : x, cb = c / ht, ca_ = c - cb * ht;
          // E: d -> O(a - (d >> 1), b - (d & 1)); O: d' -> E(a + 1 - (d' >> 1), b + 1 - (d' & 1))
          uint32_t ya = ca_, yb = cb;
          if (odd) {
            if (!(d & 2u)) ya = ca_ + 1 == ht ? 0 : ca_ + 1;
            if (!(d & 1u)) yb = cb + 1 == hx ? 0 : cb + 1;
          } else {
            if (d & 2u) ya = ca_ == 0 ? ht - 1 : ca_ - 1;
            if (d & 1u) yb = cb == 0 ? hx - 1 : cb - 1;
          }
          const uint32_t yc = yb * ht + ya;              // < nq
          y = odd ? yc : nq + yc;
          const uint32_t bit = 1u << (y & 31u);
          // a relaxed atomic load: other lanes set bits meanwhile; a stale 0 costs a test, the atomic OR below decides
          if (!(__hip_atomic_load(&map[y >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & bit)) {
            ay = slc_reflect_dot(r, sigma_of(phi[y]));
            const double prod = ax * ay;
            if (prod > 0.0) {                            // else p = 0: never bonded, no random number
              const double p = 1.0 - exp(fmin(0.0, -(beta2 * prod)));
              // the link's name from its E end: (x, d) from E, (y, 3 - d') from O
              const uint32_t e = odd ? yc : x, de = odd ? 3u - d : d;
              const U4 w = philox4x32_10(e, key.chain, key.step, ((uint32_t)P_SIGMA_BOND << 24) | (de >> 1), key.k0, key.k1);
              const double uni = (de & 1u) ? u01(w.z, w.w) : u01(w.x, w.y);
              if (uni < p) add = !(atomicOr(&map[y >> 5], bit) & bit);
            }
          }
        }
        const unsigned long long joiners = __ballot(add);
        if (joiners) {                                   // wave uniform
          const uint32_t leader = (uint32_t)__builtin_ctzll(joiners);
          uint32_t first = 0;
          if (wave_lane == leader) first = atomicAdd(&s_tail[slot], (uint32_t)__builtin_popcountll(joiners));
          first = __shfl(first, leader);
          const uint32_t pos = first + (uint32_t)__builtin_popcountll(joiners & ((1ull << wave_lane) - 1ull));
          if (add && pos < n) {
            qv[pos] = y;
            qa[pos] = ay;
          }
        }
      }
      slc_team_sync<BLOCK>();
      head = tail;
      tail = s_tail[slot];
      tail = tail < n ? tail : n;                        // the queue holds n entries (a vertex joins once)
      if (BLOCK) __syncthreads();                        // nobody appends to the next level before everybody has read the tail
    }

    for (uint32_t q = lane; q < tail; q += T) {
      const uint32_t x = qv[q];
      const double c = 2.0 * qa[q];
      const V3 s = sigma_of(phi[x]);
      phi[x] = angles_of(V3{s.x - c * r.x, s.y - c * r.y, s.z - c * r.z});
      map[x >> 5] = 0;                                   // every bit of the word that is set belongs to a member
    }
    total += tail;
    // the next update reads what this one stored (other lanes, other waves of the team): drain the stores first
    slc_team_sync<BLOCK>();
  }
  if (cluster_sites && lane == 0) cluster_sites[b] += total;
}

namespace {

struct SlcPlan {
  bool block, lds_map;
  uint32_t threads, words, grid;
  size_t lds_bytes;
};

// Launch plan: sigma_cluster.hip's with N replaced by n.  A team is one wave when there are enough chains to
// give every SIMD of the device a wave (B >= 4 x kComputeUnits), the workgroup otherwise; the bitmap sits in LDS where it
// fits.  The knobs MLMCPI_SIGMA_CLUSTER_TEAM=wave|block and MLMCPI_SIGMA_CLUSTER_BITMAP=global|lds govern both kernels.
SlcPlan slc_plan(uint32_t n, uint32_t B, const Tuning &tune) {
  SlcPlan p;
  p.words = (n + 31) / 32;
  p.block = tune.sigma_cluster_team ? tune.sigma_cluster_team == 2 : B < 4 * kComputeUnits;
  p.lds_map = !tune.sigma_cluster_map_global && p.words <= (p.block ? kSlcBlockLdsWords : kSlcWaveLdsWords);
  p.threads = p.block ? (n >= 16384 ? kSlcBlockThreads : 256u) : kSlcWaveChains * kWave;
  p.grid = p.block ? B : (B + kSlcWaveChains - 1) / kSlcWaveChains;
  p.lds_bytes = p.lds_map ? (size_t)p.words * sizeof(uint32_t) * (p.block ? 1 : kSlcWaveChains) : 0;
  return p;
}

std::mutex g_slc_attr_mutex;
bool g_slc_attr_set[64] = {false};

int slc_init_attrs() {
  int dev = 0;
  MLMCPI_HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return fail(MLMCPI_ERR_INVALID, "device index %d out of range", dev);
  std::lock_guard<std::mutex> lock(g_slc_attr_mutex);
  if (g_slc_attr_set[dev]) return MLMCPI_OK;
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_rot_cluster_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kSlcBlockLdsWords * sizeof(uint32_t)));
  g_slc_attr_set[dev] = true;
  return MLMCPI_OK;
}

int slc_check(const mlmcpi_sigma_level *level) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(level->beta > 0.0, "beta must be positive");
  return MLMCPI_OK;
}

mlmcpi_lattice_action slc_as_lattice(const mlmcpi_sigma_level *l) {
  return mlmcpi_lattice_action{MLMCPI_NONLINEAR_SIGMA, l->Mt, l->Mx, l->beta, 0.0};
}

// workspace sections: queue a [B n] double, queue vertex [B n] uint32, bitmap [B words] uint32
size_t slc_section_a(uint32_t n, uint32_t B) { return align256((size_t)B * n * sizeof(double)); }
size_t slc_section_v(uint32_t n, uint32_t B) { return align256((size_t)B * n * sizeof(uint32_t)); }
size_t slc_section_map(uint32_t n, uint32_t B) { return align256((size_t)B * ((n + 31) / 32) * sizeof(uint32_t)); }

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_sigma_level_cluster_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes) {
  if (int rc = slc_check(level)) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  if (!level->rotated) {
    const mlmcpi_lattice_action act = slc_as_lattice(level);
    return mlmcpi_sigma_cluster_workspace_bytes(&act, B, bytes);
  }
  const uint32_t n = make_level(*level).nvert();
  *bytes = slc_section_a(n, B) + slc_section_v(n, B) + slc_section_map(n, B);
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_cluster_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates,
                                    uint64_t seed, uint32_t chain0, uint32_t update0, uint32_t *d_cluster_sites, void *d_work,
                                    void *stream) {
  if (int rc = slc_check(level)) return rc;
  MLMCPI_REQUIRE(d_state && d_work && B > 0, "bad arguments");
  MLMCPI_REQUIRE((uint64_t)update0 + n_updates <= 0xFFFFFFFFull, "update counter overflows");
  if (!level->rotated) {
    const mlmcpi_lattice_action act = slc_as_lattice(level);
    return mlmcpi_sigma_cluster_draw(&act, d_state, B, n_updates, seed, chain0, update0, d_cluster_sites, d_work, stream);
  }
  if (int rc = slc_init_attrs()) return rc;
  const SigmaLevel L = make_level(*level);
  const uint32_t n = L.nvert();
  const SlcPlan p = slc_plan(n, B, tuning());
  char *w = (char *)d_work;
  double *qa = (double *)w;
  uint32_t *qv = (uint32_t *)(w + slc_section_a(n, B));
  uint32_t *map = (uint32_t *)(w + slc_section_a(n, B) + slc_section_v(n, B));
  const RngKey key = make_key(seed, chain0, update0);
  const hipStream_t st = as_stream(stream);
#define MLMCPI_SLC_LAUNCH(BLOCK, LDS)                                                                                          \
  hipLaunchKernelGGL((sigma_rot_cluster_kernel<BLOCK, LDS>), dim3(p.grid), dim3(p.threads), p.lds_bytes, st, (double2 *)d_state, L, \
                     2.0 * level->beta, B, n_updates, key, qv, qa, map, p.words, d_cluster_sites)
  if (p.block && p.lds_map) MLMCPI_SLC_LAUNCH(true, true);
  else if (p.block) MLMCPI_SLC_LAUNCH(true, false);
  else if (p.lds_map) MLMCPI_SLC_LAUNCH(false, true);
  else MLMCPI_SLC_LAUNCH(false, false);
#undef MLMCPI_SLC_LAUNCH
  MLMCPI_LAUNCH_CHECK("sigma_rot_cluster_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
