// sigma_cluster_device.hpp -- what the cluster samplers of the O(3) nonlinear sigma model share (sigma_cluster.hip: Wolff,
// sigma_sw*.hip: Swendsen-Wang; each on the unrotated lattice and on the rotated level of the CoarsenRotate hierarchy): the
// embedding (normal, bond rule, reflection), the team's phase fence, the two geometries the kernels are instantiated on, and
// the fixed point, the weights and the lag scale of the improved estimators.  What only Swendsen-Wang uses is in
// sigma_sw_device.hpp, what only Wolff uses in sigma_cluster.hip.  Includes sigma_device.hpp (through sigma_level_device.hpp),
// so the including file is compiled without fp contraction.
#pragma once
#include "sigma_level_device.hpp"

namespace mlmcpi {

constexpr uint32_t kClusterThreads = 256;        // Wolff, team = wave: four chains per workgroup; SW tiled plan: every launch but the last
constexpr uint32_t kClusterBlockThreads = 1024;  // Wolff, team = workgroup; the fixed configuration of sw_finish; the SW chain plan's workgroup
constexpr double kSwFix = 4294967296.0;          // 2^32

// ---- host: what both samplers ask of a level ---------------------------------------------------------------------------------
inline int check_cluster_level(const mlmcpi_sigma_level *level) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(level->beta > 0.0, "beta must be positive");
  return MLMCPI_OK;
}

// an unrotated level IS the lattice and takes the lattice's entry point
inline mlmcpi_lattice_action level_as_lattice(const mlmcpi_sigma_level *l) {
  return mlmcpi_lattice_action{MLMCPI_NONLINEAR_SIGMA, l->Mt, l->Mx, l->beta, 0.0};
}

// ---- the embedding ---------------------------------------------------------------------------------------------------------
// the reflection normal of an update: (u, v) of (site 0, sub 0) -> r_z = 1 - 2 u, azimuth 2 pi v - pi.  Wolff draws it under
// P_SIGMA_REFLECT, Swendsen-Wang under P_SIGMA_SW_REFLECT.
__device__ __forceinline__ V3 reflection_normal(const RngKey &key, uint32_t purpose) {
  double u, v;
  rng_uniforms(key, 0, purpose, 0, u, v);
  const double rz = 1.0 - 2.0 * u, t = 1.0 - rz * rz, rho = t > 0.0 ? sqrt(t) : 0.0;
  double sa, ca;
  sincos(kTwoPi * v - kPi, &sa, &ca);
  return V3{rho * ca, rho * sa, rz};
}

// the bond probability of a link with prod = a_x a_y > 0 (prod <= 0: p = 0, never bonded, and no caller asks)
__device__ __forceinline__ double bond_probability(double prod, double beta2) { return 1.0 - exp(fmin(0.0, -(beta2 * prod))); }

// the product first: the same bits from either end of the link
__device__ __forceinline__ bool bonded(double ax, double ay, double beta2, double uni) {
  const double prod = ax * ay;
  if (!(prod > 0.0)) return false;                       // p = 0: never bonded
  return uni < bond_probability(prod, beta2);
}

// sigma' = sigma - 2 a r in the canonical form (sigma2d.hip)
__device__ __forceinline__ double2 reflected(const V3 &s, double a, const V3 &r) {
  const double c = 2.0 * a;
  return angles_of(V3{s.x - c * r.x, s.y - c * r.y, s.z - c * r.z});
}

// What orders one phase of a team behind the one before it: the phase's stores (state, queue, bitmap) drained and, for a
// team of several waves, the barrier.  A team of one wave runs in lockstep and needs the drain only.
template <bool BLOCK>
__device__ __forceinline__ void team_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  if (BLOCK) __syncthreads();
  else __builtin_amdgcn_wave_barrier();
}

// ---- the geometries ---------------------------------------------------------------------------------------------------------
// A geometry answers what the Swendsen-Wang kernels and the host ask and nothing else: the number of vertices, which vertices
// own links, how many each, their far ends and their bond bits.  The chain kernel of sigma_sw_chain.hip is written once and
// instantiated on LatticeGeometry and RotatedGeometry; the tile front ends of sigma_sw_tiled.hip (bond + label, merge) differ
// for real and stay one per geometry, and so do the Wolff kernels of sigma_cluster.hip (the reason is given there), which walk
// the same links.

// The unrotated lattice: vertex l = Mt j + i; link (l, 0) joins l to its +i neighbour, link (l, 1) to its +j neighbour (periodic,
// 2 N links; on an extent of 2 the two links between a pair are two links with a uniform each).  One Philox call per vertex:
// site l, sub 0, u decides link (l, 0), v decides link (l, 1).
struct LatticeGeometry {
  uint32_t Mt, Mx;
  static constexpr uint32_t kOwnedLinks = 2;
  static constexpr bool kStructure = false;
  static constexpr bool kRoots = false;
  __host__ __device__ uint32_t nvert() const { return Mt * Mx; }
  __host__ __device__ uint32_t nowners() const { return Mt * Mx; }
  // the structure sums: the periodic extent of direction d (0: t, 1: x) and the position of vertex l along it, l at (i, j)
  __host__ __device__ uint32_t extent(uint32_t d) const { return d ? Mx : Mt; }
  __device__ __forceinline__ uint32_t position(uint32_t l, uint32_t d) const { return d ? l / Mt : l % Mt; }

  __device__ __forceinline__ void far_ends(uint32_t l, uint32_t (&y)[2]) const {
    const uint32_t i = l % Mt, j = l / Mt;
    y[0] = i + 1 == Mt ? l - i : l + 1;
    y[1] = j + 1 == Mx ? i : l + Mt;
  }

  // (bond of link (l, 0), bond of link (l, 1)) as bits 0 and 1
  static __device__ __forceinline__ uint32_t bonds(const RngKey &key, uint32_t l, double a, double a_right, double a_up, double beta2) {
    const U4 w = philox4x32_10(l, key.chain, key.step, (uint32_t)P_SIGMA_SW_BOND << 24, key.k0, key.k1);
    return (bonded(a, a_right, beta2, u01(w.x, w.y)) ? 1u : 0u) | (bonded(a, a_up, beta2, u01(w.z, w.w)) ? 2u : 0u);
  }
  // the form the chain kernel calls on either geometry: ay[d] = a of the far end of link (l, d).  The bond + label kernel keeps
  // the scalar form: built through this one it comes out with its LDS reads in another order.
  static __device__ __forceinline__ uint32_t bonds(const RngKey &key, uint32_t l, double a, const double (&ay)[2], double beta2) {
    return bonds(key, l, a, ay[0], ay[1], beta2);
  }
};

// The rotated level (sigma_level_device.hpp): n = 2 q vertices, plane E then plane O of ht x hx each, index p q + ht b + a.  It is
// bipartite: every link has exactly one E end, so the 2 n links are named (e, d) with e an E vertex (e < q) and d its direction
// in the reference's order: E(a, b) -> O(a, b), O(a, b-1), O(a-1, b), O(a-1, b-1).  Seen from O(a, b), direction d' -> E(a+1, b+1),
// E(a+1, b), E(a, b+1), E(a, b) crosses link (neighbour, 3 - d').  Where a plane extent is 1 several of the four neighbours of a
// vertex are one vertex; those are distinct links with a uniform each.  Two Philox calls per E vertex: site e, sub d >> 1, u
// decides link (e, d) for d even, v for d odd.
struct RotatedGeometry {
  uint32_t ht, hx, q;  // q = ht hx
  static constexpr uint32_t kOwnedLinks = 4;
  static constexpr bool kStructure = false;
  static constexpr bool kRoots = false;
  explicit RotatedGeometry(const SigmaLevel &L) : ht(L.ht), hx(L.hx), q(L.q) {}
  __host__ __device__ uint32_t nvert() const { return 2 * q; }
  __host__ __device__ uint32_t nowners() const { return q; }
  // the structure sums: the level's extents Mt = 2 ht, Mx = 2 hx; plane p, cell (a, b) sits at (i, j) = (2 a + p, 2 b + p), the
  // slice assignment of mlmcpi_sigma_level_correlator
  __host__ __device__ uint32_t extent(uint32_t d) const { return 2 * (d ? hx : ht); }
  __device__ __forceinline__ uint32_t position(uint32_t l, uint32_t d) const {
    const uint32_t p = l >= q ? 1u : 0u, c = l - p * q;
    return 2 * (d ? c / ht : c % ht) + p;
  }

  __device__ __forceinline__ void far_ends(uint32_t e, uint32_t (&y)[4]) const {
    const uint32_t cb = e / ht, ca = e - cb * ht;
    const uint32_t am = ca == 0 ? ht - 1 : ca - 1, bm = cb == 0 ? hx - 1 : cb - 1;
    y[0] = q + cb * ht + ca;
    y[1] = q + bm * ht + ca;
    y[2] = q + cb * ht + am;
    y[3] = q + bm * ht + am;
  }

  // the bonds of the links (e, 0) .. (e, 3) as bits 0 .. 3; ao[d] = a of the O end of link (e, d)
  static __device__ __forceinline__ uint32_t bonds(const RngKey &key, uint32_t e, double a, const double (&ao)[4], double beta2) {
    const U4 w0 = philox4x32_10(e, key.chain, key.step, (uint32_t)P_SIGMA_SW_BOND << 24, key.k0, key.k1);
    const U4 w1 = philox4x32_10(e, key.chain, key.step, ((uint32_t)P_SIGMA_SW_BOND << 24) | 1u, key.k0, key.k1);
    return (bonded(a, ao[0], beta2, u01(w0.x, w0.y)) ? 1u : 0u) | (bonded(a, ao[1], beta2, u01(w0.z, w0.w)) ? 2u : 0u) |
           (bonded(a, ao[2], beta2, u01(w1.x, w1.y)) ? 4u : 0u) | (bonded(a, ao[3], beta2, u01(w1.z, w1.w)) ? 8u : 0u);
  }
};

// ---- the improved estimators: the fixed point, the weights, the lags -------------------------------------------------------------
// a = r . sigma in 64-bit fixed point: sums of q(a) are integer sums, the same bits in every order
__device__ __forceinline__ long long sw_fixed(double a) { return llrint(a * kSwFix); }

// the weights of a vertex at position x of a periodic direction of extent M: s = sin(2 pi x / M), c = cos(2 pi x / M).  The one
// place that forms them, from the integers: both plans and both geometries get the same bits, and M = 2 gives exactly 0 and +-1.
__device__ __forceinline__ void sw_phase(uint32_t x, uint32_t M, double &s, double &c) { sincospi(2.0 * (double)x / (double)M, &s, &c); }

// The lag accumulators of the improved correlators (Swendsen-Wang: sigma_sw_correlator.hip, Wolff: sigma_cluster.hip), on a
// geometry of N vertices and extents M_0, M_1.  n_out = (M_0 / 2 + 1) + (M_1 / 2 + 1): the lags 0 .. M_d / 2 of direction t, then of
// x, the layout of mlmcpi_sigma_level_correlator.  An accumulator sums llrint(P P' 2^(s - 64)) over the pairs of slice sums
// P = sum of q(a) at its lag; s is the largest scale that keeps it inside 63 bits, min(32, 62 - ceil(log2(N N_slice))) with
// N_slice = N / min(M_0, M_1) the vertices of the larger slice: sum_i sum_C |P(i)| |P(i + tau)| <= sum_i N_slice sum_C n_C(i) = N
// N_slice (|a| <= 1, n_C(i) the vertices of C in slice i), so |acc| <= 2^62 + N / 2 with the roundings of the terms.  The sum over
// one cluster (Wolff) is at most the sum over all of them.
struct SwLagScale {
  uint32_t n_out, s;
};

inline SwLagScale sw_lag_scale(uint32_t N, uint32_t M0, uint32_t M1) {
  const uint64_t bound = (uint64_t)N * (N / (M0 < M1 ? M0 : M1));
  uint32_t lb = 0;
  while ((1ull << lb) < bound) ++lb;
  return SwLagScale{M0 / 2 + M1 / 2 + 2, 62 - lb < 32 ? 62 - lb : 32};
}

}  // namespace mlmcpi
