// sigma_topology.hip -- the geometric (Berg-Luescher) topological charge of an O(3) sigma-model state on a level, rotated or not,
// and the susceptibility Q^2 / n (include/mlmcpi_hip.h: mlmcpi_sigma_level_topological_charge).
//
//   A(a, b, c) = 2 atan2(a . (b x c), 1 + a . b + b . c + c . a)      the signed area of the spherical triangle (a, b, c)
//   Q = (1 / 4 pi) sum over faces [A(c1, c2, c3) + A(c1, c3, c4)],    chi = Q^2 / n
//
// Faces.  Plain level: one per vertex (i, j), corners c1 .. c4 = (i, j), (i+1, j), (i+1, j+1), (i, j+1).  Rotated level: one per
// site (i, j) with i + j odd, corners c1 .. c4 = W, S, E, N = (i-1, j), (i, j-1), (i+1, j), (i, j+1), all level vertices.  In the
// planes of sigma_level_device.hpp (E(a, b) = (2a, 2b), O(a, b) = (2a+1, 2b+1)) a cell (a, b) owns two faces:
//   site (2a+1, 2b):  W, S, E, N = E(a, b),   O(a, b-1), E(a+1, b), O(a, b)
//   site (2a, 2b+1):  W, S, E, N = O(a-1, b), E(a, b),   O(a, b),   E(a, b+1)
// so n / 2 cells carry n faces.  Everything is periodic.
//
// Two launches, the state is read ONCE:
//   1. sigma_topo_tile_kernel: a workgroup takes a tile of 32 x 32 plane cells (plain: vertices) of one chain, clipped at the upper
//      edges of the plane.  Staging: one sincos pair per vertex into LDS, three SoA planes of doubles per vertex plane, (tw + 1) x
//      (th + 1) entries each: the tile and the one-vertex halo its faces reach, wrapped periodically.  Plain and E: local (la, lb)
//      is the plane entry (a0 + la, b0 + lb); O is staged one cell lower, local (la, lb) = O(a0 - 1 + la, b0 - 1 + lb), so that
//      both planes of a rotated tile have the same extent.  The row stride is 33 doubles: the 32 lanes of a ds_read_b64 that walk a
//      row, and on into the next, touch 32 different bank pairs.  Faces: thread t takes the cells t, t + 256, .. of the tile in
//      ascending order (cell = tw cb + ca), on a rotated level the face of site (2a+1, 2b) before that of (2a, 2b+1); per face 5
//      dot products (c1 . c3 serves both triangles), 2 triple products, 2 atan2.  block_sum adds the threads; the tile's partial
//      goes to partial[chain][tile].
//   2. sigma_topo_finish_kernel: one workgroup per chain adds the tile partials (chain_sum) and writes Q, Q^2 / n and, with d_acc,
//      the record_sample moments of chi.
// Tile, thread -> cell map and the number of partials are functions of (Mt, Mx, rotated) alone and there are no atomics: a chain's
// outputs are the same bits for every batch size, every split of the chains over calls, every stream, and whichever of d_q, d_chi
// and d_acc are asked for.  Workgroups of both launches are one linear index (chain x tile; chain) laid over grid x and past it y.
// The two atan2 of a face stay two: the product of the triangles' complex numbers would lose the 2 pi the sum can wind by.
#include "internal.hpp"

#include "sigma_topology_device.hpp"  // the face code; fp contraction is off from here on

namespace mlmcpi {

template <int ROT>
__global__ void __launch_bounds__(kTopoThreads)
    sigma_topo_tile_kernel(TopoPlan G, uint64_t nblocks, const double2 *__restrict__ phi, double *__restrict__ partial) {
  constexpr uint32_t NP = ROT ? 2 : 1;
  __shared__ double sig[NP * 3 * kTopoPlane];
  __shared__ double red[kTopoThreads / kWave];
  const uint64_t wg = topo_block();
  if (wg >= nblocks) return;
  const uint32_t tid = threadIdx.x;
  const TopoTile T = topo_tile(G, (uint32_t)(wg % G.tiles));
  const double2 *s = phi + (size_t)(wg / G.tiles) * G.nvert;

  topo_stage<ROT>(G, T, sig, [s](size_t l) { return sigma_of(s[l]); });
  __syncthreads();

  // topo_faces<ROT>(T, sig), written out: called here it flips the polarity of one branch of block_sum, and this kernel's
  // instructions are pinned (tools/kernel_digest.py)
  const uint32_t tw = T.tw, th = T.th;
  double acc[1] = {0.0};
  for (uint32_t t = tid; t < tw * th; t += kTopoThreads) {
    const uint32_t c = (t / tw) * kTopoLd + t % tw;
    if constexpr (ROT) {
      const double *E = sig, *O = sig + 3 * kTopoPlane;
      const V3 e00 = topo_load(E, c), e10 = topo_load(E, c + 1), e01 = topo_load(E, c + kTopoLd);
      const V3 o10 = topo_load(O, c + 1), o01 = topo_load(O, c + kTopoLd), o11 = topo_load(O, c + kTopoLd + 1);
      acc[0] += topo_face(e00, o10, e10, o11);  // site (2a+1, 2b)
      acc[0] += topo_face(o01, e00, o11, e01);  // site (2a, 2b+1)
    } else {
      acc[0] += topo_face(topo_load(sig, c), topo_load(sig, c + 1), topo_load(sig, c + kTopoLd + 1), topo_load(sig, c + kTopoLd));
    }
  }
  block_sum<1>(acc, red);
  if (tid == 0) partial[wg] = acc[0];
}

// workgroup w < n_chains: Q = sum of the chain's tile partials / 2 pi, chi = Q^2 / n
__global__ void __launch_bounds__(kTopoThreads)
    sigma_topo_finish_kernel(const double *__restrict__ partial, uint32_t tiles, uint64_t n_chains, double n, double *__restrict__ q,
                             double *__restrict__ chi, double *__restrict__ acc) {
  __shared__ double red[kTopoThreads / kWave];
  const uint64_t b = topo_block();
  if (b >= n_chains) return;
  double v[1];
  chain_sum<1>(partial + b * tiles, tiles, v, red);
  if (threadIdx.x != 0) return;
  const double Q = v[0] / kTwoPi, X = (Q * Q) / n;
  if (q) q[b] = Q;
  if (chi) chi[b] = X;
  if (acc) record_moments(acc + 5 * b, X);
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_sigma_level_topological_charge(const mlmcpi_sigma_level *level, const double *d_state, uint32_t n_chains, double *d_q,
                                          double *d_chi, double *d_acc, void *stream) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(d_state, "the topological charge needs a state (d_state is NULL)");
  MLMCPI_REQUIRE(d_q || d_chi, "the topological charge needs d_q or d_chi (both are NULL)");
  MLMCPI_REQUIRE(n_chains > 0, "the topological charge needs n_chains > 0");
  const SigmaLevel L = make_level(*level);
  const TopoPlan G = topo_plan(L);
  const uint64_t blocks = (uint64_t)n_chains * G.tiles;
  MLMCPI_REQUIRE(blocks <= kTopoMaxBlocks, "the topological charge takes at most %llu workgroups per launch (these chains need %llu)",
                 (unsigned long long)kTopoMaxBlocks, (unsigned long long)blocks);
  hipStream_t st = as_stream(stream);
  void *part = nullptr;
  if (int rc = scratch((size_t)blocks * sizeof(double), &part, st)) return rc;
  if (L.rot)
    hipLaunchKernelGGL(sigma_topo_tile_kernel<1>, topo_grid(blocks), dim3(kTopoThreads), 0, st, G, blocks, (const double2 *)d_state, (double *)part);
  else
    hipLaunchKernelGGL(sigma_topo_tile_kernel<0>, topo_grid(blocks), dim3(kTopoThreads), 0, st, G, blocks, (const double2 *)d_state, (double *)part);
  MLMCPI_LAUNCH_CHECK("sigma_topo_tile_kernel");
  hipLaunchKernelGGL(sigma_topo_finish_kernel, topo_grid(n_chains), dim3(kTopoThreads), 0, st, (const double *)part, G.tiles, (uint64_t)n_chains,
                     (double)G.nvert, d_q, d_chi, d_acc);
  MLMCPI_LAUNCH_CHECK("sigma_topo_finish_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
