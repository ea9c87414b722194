// sigma_field.hip -- a field of unit vectors of the O(3) sigma model on a level, rotated or not, in a caller's workspace
// (sigma_field_device.hpp): the workspace layout, the map from a state of angles and back, and what is measured on the field --
// charge, susceptibility and bond energy.  What smooths the field between two measurements is a smoother's own
// (sigma_cooling.hip, sigma_flow.hip; the driver of both is sigma_smooth.hip).
// Kernels: stage (sigma_of(angles) -> a vector buffer, one sincos pair per vertex) and angles (the map back); charge<ROT> (the
// tile, staging, faces and sum order of sigma_topo_tile_kernel, sigma_topology_device.hpp, fed from the vector buffer), energy<ROT>
// (sigma_l . Delta_l summed per group of 256 consecutive vertices, block_sum) and finish (one workgroup per chain: chain_sum of
// both kinds of partials -> Q, chi, E).
// The sums are functions of the level alone.  No atomics; workgroups of every launch ride one linear index over grid x and then y
// (topo_grid).
#include "internal.hpp"

#include "sigma_field_device.hpp"  // the field's layout and the face code; fp contraction is off from here on

namespace mlmcpi {

// workgroup (chain, group g of 256 vertices): the field of a state of angles
__global__ void __launch_bounds__(kGroup)
    sigma_field_stage_kernel(uint32_t n, uint32_t ngroups, uint64_t nblocks, const double2 *__restrict__ phi, double *__restrict__ vec) {
  const uint64_t wg = topo_block();
  if (wg >= nblocks) return;
  const uint64_t b = wg / ngroups;
  const uint32_t l = (uint32_t)(wg % ngroups) * kGroup + threadIdx.x;
  if (l < n) field_store(vec + b * 3 * n, n, l, sigma_of(phi[b * n + l]));
}

// the same map back: the angles of the field
__global__ void __launch_bounds__(kGroup)
    sigma_field_angles_kernel(uint32_t n, uint32_t ngroups, uint64_t nblocks, const double *__restrict__ vec, double2 *__restrict__ phi) {
  const uint64_t wg = topo_block();
  if (wg >= nblocks) return;
  const uint64_t b = wg / ngroups;
  const uint32_t l = (uint32_t)(wg % ngroups) * kGroup + threadIdx.x;
  if (l < n) phi[b * n + l] = angles_of(field_fetch(vec + b * 3 * n, n, l));
}

// ---- measurement ---------------------------------------------------------------------------------------------------------------
// sigma_topo_tile_kernel on the vector buffer: partial[chain][tile]
template <int ROT>
__global__ void __launch_bounds__(kTopoThreads)
    sigma_field_charge_kernel(TopoPlan G, uint64_t nblocks, const double *__restrict__ vec, double *__restrict__ partial) {
  constexpr uint32_t NP = ROT ? 2 : 1;
  __shared__ double sig[NP * 3 * kTopoPlane];
  __shared__ double red[kTopoThreads / kWave];
  const uint64_t wg = topo_block();
  if (wg >= nblocks) return;
  const TopoTile T = topo_tile(G, (uint32_t)(wg % G.tiles));
  const double *s = vec + (wg / G.tiles) * 3 * G.nvert;
  const uint32_t n = G.nvert;

  topo_stage<ROT>(G, T, sig, [s, n](size_t l) { return field_fetch(s, n, l); });
  __syncthreads();

  double acc[1] = {topo_faces<ROT>(T, sig)};
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) partial[wg] = acc[0];
}

// workgroup (chain, group g): sum over the vertices l of the group of sigma_l . Delta_l -> partial[chain][g]
template <int ROT>
__global__ void __launch_bounds__(kGroup)
    sigma_field_energy_kernel(SigmaLevel L, uint32_t ngroups, uint64_t nblocks, const double *__restrict__ vec, double *__restrict__ partial) {
  __shared__ double red[kGroup / kWave];
  const uint64_t wg = topo_block();
  if (wg >= nblocks) return;
  const uint32_t n = L.nvert(), l = (uint32_t)(wg % ngroups) * kGroup + threadIdx.x;
  const double *s = vec + (wg / ngroups) * 3 * n;
  double acc[1] = {0.0};
  if (l < n) {
    uint32_t nb[4];
    if constexpr (ROT) {
      const uint32_t p = l >= L.q ? 1 : 0, r = l - p * L.q, a = r % L.ht, b = r / L.ht;
      if (p) {  // O(a, b): E(a+1, b+1), E(a+1, b), E(a, b+1), E(a, b)
        const uint32_t ap = a + 1 == L.ht ? 0 : a + 1, bp = b + 1 == L.hx ? 0 : b + 1;
        nb[0] = bp * L.ht + ap;
        nb[1] = b * L.ht + ap;
        nb[2] = bp * L.ht + a;
        nb[3] = b * L.ht + a;
      } else {  // E(a, b): O(a, b), O(a, b-1), O(a-1, b), O(a-1, b-1)
        const uint32_t am = a == 0 ? L.ht - 1 : a - 1, bm = b == 0 ? L.hx - 1 : b - 1;
        nb[0] = L.q + b * L.ht + a;
        nb[1] = L.q + bm * L.ht + a;
        nb[2] = L.q + b * L.ht + am;
        nb[3] = L.q + bm * L.ht + am;
      }
    } else {
      const uint32_t i = l % L.Mt, j = l / L.Mt;
      nb[0] = j * L.Mt + (i + 1 == L.Mt ? 0 : i + 1);
      nb[1] = j * L.Mt + (i == 0 ? L.Mt - 1 : i - 1);
      nb[2] = (j + 1 == L.Mx ? 0 : j + 1) * L.Mt + i;
      nb[3] = (j == 0 ? L.Mx - 1 : j - 1) * L.Mt + i;
    }
    acc[0] = dot3(field_fetch(s, n, l), add4(field_fetch(s, n, nb[0]), field_fetch(s, n, nb[1]), field_fetch(s, n, nb[2]), field_fetch(s, n, nb[3])));
  }
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) partial[wg] = acc[0];
}

// workgroup b < n_chains, column k of the outputs: Q = sum of the tile partials / 2 pi, chi = Q^2 / n, E = 2 n - sum of the
// group partials / 2
__global__ void __launch_bounds__(kGroup)
    sigma_field_finish_kernel(const double *__restrict__ part_q, uint32_t tiles, const double *__restrict__ part_e, uint32_t ngroups,
                             uint64_t n_chains, double n, uint32_t n_depths, uint32_t k, double *__restrict__ q, double *__restrict__ chi,
                             double *__restrict__ energy) {
  __shared__ double red[kGroup / kWave];
  const uint64_t b = topo_block();
  if (b >= n_chains) return;
  double v[1];
  if (q || chi) {
    chain_sum<1>(part_q + b * tiles, tiles, v, red);
    if (threadIdx.x == 0) {
      const double Q = v[0] / kTwoPi;
      if (q) q[b * n_depths + k] = Q;
      if (chi) chi[b * n_depths + k] = (Q * Q) / n;
    }
  }
  if (energy) {
    __syncthreads();  // red is used again
    chain_sum<1>(part_e + b * ngroups, ngroups, v, red);
    if (threadIdx.x == 0) energy[b * n_depths + k] = 2.0 * n - 0.5 * v[0];
  }
}

// ---- the host side (sigma_field_device.hpp) ------------------------------------------------------------------------------------
FieldWork field_work(const SigmaLevel &L, uint32_t n_chains) {
  FieldWork w;
  w.ngroups = (L.nvert() + kGroup - 1) / kGroup;
  w.vec = align256((size_t)n_chains * 3 * L.nvert() * sizeof(double));
  w.part_q = align256((size_t)n_chains * topo_plan(L).tiles * sizeof(double));
  w.part_e = align256((size_t)n_chains * w.ngroups * sizeof(double));
  w.total = 2 * w.vec + w.part_q + w.part_e;
  return w;
}

int field_stage(const SigmaLevel &L, const FieldWork &w, uint32_t n_chains, const double *d_state, double *vec, hipStream_t st) {
  const uint64_t vblocks = (uint64_t)n_chains * w.ngroups;
  hipLaunchKernelGGL(sigma_field_stage_kernel, topo_grid(vblocks), dim3(kGroup), 0, st, L.nvert(), w.ngroups, vblocks, (const double2 *)d_state, vec);
  MLMCPI_LAUNCH_CHECK("sigma_field_stage_kernel");
  return MLMCPI_OK;
}

int field_measure(const SigmaLevel &L, const FieldWork &w, uint32_t n_chains, const double *vec, double *part_q, double *part_e,
                  uint32_t n_cols, uint32_t k, double *d_q, double *d_chi, double *d_energy, hipStream_t st) {
  const TopoPlan G = topo_plan(L);
  const uint64_t vblocks = (uint64_t)n_chains * w.ngroups, qblocks = (uint64_t)n_chains * G.tiles;
  if (d_q || d_chi) {
    if (L.rot) hipLaunchKernelGGL(sigma_field_charge_kernel<1>, topo_grid(qblocks), dim3(kTopoThreads), 0, st, G, qblocks, vec, part_q);
    else hipLaunchKernelGGL(sigma_field_charge_kernel<0>, topo_grid(qblocks), dim3(kTopoThreads), 0, st, G, qblocks, vec, part_q);
    MLMCPI_LAUNCH_CHECK("sigma_field_charge_kernel");
  }
  if (d_energy) {
    if (L.rot) hipLaunchKernelGGL(sigma_field_energy_kernel<1>, topo_grid(vblocks), dim3(kGroup), 0, st, L, w.ngroups, vblocks, vec, part_e);
    else hipLaunchKernelGGL(sigma_field_energy_kernel<0>, topo_grid(vblocks), dim3(kGroup), 0, st, L, w.ngroups, vblocks, vec, part_e);
    MLMCPI_LAUNCH_CHECK("sigma_field_energy_kernel");
  }
  hipLaunchKernelGGL(sigma_field_finish_kernel, topo_grid(n_chains), dim3(kGroup), 0, st, (const double *)part_q, G.tiles, (const double *)part_e,
                     w.ngroups, (uint64_t)n_chains, (double)L.nvert(), n_cols, k, d_q, d_chi, d_energy);
  MLMCPI_LAUNCH_CHECK("sigma_field_finish_kernel");
  return MLMCPI_OK;
}

int field_angles(const SigmaLevel &L, const FieldWork &w, uint32_t n_chains, const double *vec, double *d_out, hipStream_t st) {
  const uint64_t vblocks = (uint64_t)n_chains * w.ngroups;
  hipLaunchKernelGGL(sigma_field_angles_kernel, topo_grid(vblocks), dim3(kGroup), 0, st, L.nvert(), w.ngroups, vblocks, vec, (double2 *)d_out);
  MLMCPI_LAUNCH_CHECK("sigma_field_angles_kernel");
  return MLMCPI_OK;
}

}  // namespace mlmcpi
