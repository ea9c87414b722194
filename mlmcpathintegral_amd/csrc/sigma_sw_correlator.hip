// sigma_sw_correlator.hip -- the cluster-improved time-slice correlator of the Swendsen-Wang update of the O(3) nonlinear sigma
// model (mlmcpi_sigma_level_sw_correlator_draw; sigma_sw.hip has the update and the draw): per cluster,
// direction and slice the sum of q(a) in a hash table keyed by (root, slice), per cluster and lag the products of those sums
// in a 64-bit fixed-point accumulator, added to corr[b][n_out] update by update.  Its own kernels are the three below, the same
// for both plans and both geometries; under the chain plan sigma_sw_chain_kernel<WithRoots<Geometry>> leaves roots and q(a)
// where the tiled plan has them.  The instances of the plain and the structure draw are untouched.
#include "sigma_sw_host.hpp"

#include "sigma_sw_device.hpp"  // fp contraction is off from here on

namespace mlmcpi {

// After an update of either plan the workspace holds a label array whose walk ends at every vertex's final root (tiled: the
// parents of launch 3; chain: the roots themselves) and q(a) of the field before the update.  Three launches follow, and every
// sum in them is an integer sum: no order matters.
//
// (1) one lane per vertex: q(a) onto P_C,d(x_d(l)) of the chain's table of either direction.  Every lane stays to the end.
template <class Geometry>
__global__ void __launch_bounds__(kClusterThreads)
    sigma_sw_slice_sum_kernel(Geometry g, uint32_t blocks, const uint32_t *label_all, const long long *qa_all, unsigned long long *table_all,
                              uint32_t lg, uint32_t *count_all, uint32_t *status) {
  const uint32_t N = g.nvert(), b = blockIdx.x / blocks, l = (blockIdx.x % blocks) * kClusterThreads + threadIdx.x;
  const bool active = l < N;
  bool capped = false;
  uint32_t root = 0;
  long long v = 0;
  if (active) {
    root = uf_find<kUfPlain>(label_all + (size_t)b * N, l, N, capped);
    v = qa_all[(size_t)b * N + l];
  }
#pragma unroll
  for (uint32_t d = 0; d < 2; ++d)
    sw_slice_add_combined(table_all + ((size_t)(2 * b + d) << (lg + 1)), lg, count_all + (size_t)(2 * b + d) * N, root,
                          active ? g.position(l, d) : 0u, active, v, capped);
  if (capped) atomicOr(status, 1u);
}

// (2) one lane per slot of the table of (chain, direction), kSwPairBatches slots in turn: an occupied slot (C, i, P) meets
// (C, (i + tau) mod M) for tau = 0 .. min(M / 2, w - 1), w the number of slices C occupies in that direction.  A larger lag finds
// nothing: a link changes the slice index by at most 1 on either geometry, so the slices of a cluster are an arc of the ring,
// and one that holds i and i + tau, tau <= M / 2, holds tau + 1 slices at least.  The term llrint(P P' 2^(s - 64)) (the product of
// the two integers in double, then the exact scale) goes onto acc[chain][direction][tau]: the lanes of a wave are added up
// first, the waves and batches of a workgroup meet in LDS for the lags below kSwPairLdsLags (where nearly every term falls:
// without that stage every wave of a chain sends its atomics to the same few words), and the workgroup sends one atomic per
// lag it holds; a lag beyond goes to the accumulator directly.  The loop over the lags runs to the wave's largest, so that its
// ballots and shuffles see all lanes.  Integer sums throughout: no order matters.
constexpr uint32_t kSwPairBatches = 16;    // slots a lane takes in turn
constexpr uint32_t kSwPairLdsLags = 128;   // lags a workgroup sums in LDS before it adds to the accumulator

__global__ void __launch_bounds__(kClusterThreads)
    sigma_sw_slice_pair_kernel(const unsigned long long *table_all, uint32_t lg, const uint32_t *count_all, uint32_t N, uint32_t M0, uint32_t M1,
                               uint32_t blocks, double scale, long long *acc_all, uint32_t *status) {
  __shared__ long long part[kSwPairLdsLags];
  const uint32_t bd = blockIdx.x / blocks, d = bd & 1u, slot0 = (blockIdx.x % blocks) * (kClusterThreads * kSwPairBatches) + threadIdx.x;
  const uint32_t lane = threadIdx.x & (kWave - 1), M = d ? M1 : M0;
  const unsigned long long *table = table_all + ((size_t)bd << (lg + 1));
  long long *acc = acc_all + (size_t)(bd >> 1) * (M0 / 2 + M1 / 2 + 2) + (d ? M0 / 2 + 1 : 0);
  bool capped = false;
  if (threadIdx.x < kSwPairLdsLags) part[threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t batch = 0; batch < kSwPairBatches; ++batch) {
    const uint32_t slot = slot0 + batch * kClusterThreads;
    const unsigned long long key = slot < (1u << lg) ? table[2 * (size_t)slot] : 0ull;
    const uint32_t root = (uint32_t)(key >> 32), i = (uint32_t)key - 1u;
    uint32_t ntau = 0;
    long long Pq = 0;
    if (key) {
      const uint32_t w = count_all[(size_t)bd * N + root];
      ntau = (w - 1u < M / 2 ? w - 1u : M / 2) + 1u;
      Pq = (long long)table[2 * (size_t)slot + 1];
    }
    const double P = (double)Pq;
    uint32_t tmax = ntau;
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)tmax, off);
      tmax = o > tmax ? o : tmax;
    }
    for (uint32_t tau = 0; tau < tmax; ++tau) {
      long long term = 0;
      if (tau < ntau) {
        uint32_t k = i + tau;
        if (k >= M) k -= M;
        const long long Q = tau ? sw_slice_lookup(table, lg, root, k, capped) : Pq;
        term = llrint((P * (double)Q) * scale);
      }
      const unsigned long long m = __ballot(term != 0);
      if (!m) continue;
      if (__builtin_popcountll(m) > 1) {
        for (int off = kWave / 2; off > 0; off >>= 1) term += __shfl_xor(term, off);
        if (lane != (uint32_t)__builtin_ctzll(m)) term = 0;
      }
      if (term) {
        if (tau < kSwPairLdsLags) __hip_atomic_fetch_add(part + tau, term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else __hip_atomic_fetch_add(acc + tau, term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kSwPairLdsLags && threadIdx.x <= M / 2 && part[threadIdx.x])
    __hip_atomic_fetch_add(acc + threadIdx.x, part[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (capped) atomicOr(status, 1u);
}

// (3) one lane per (chain, lag): corr[b][k] += (acc 2^-s) 3 / N
__global__ void __launch_bounds__(kClusterThreads)
    sigma_sw_slice_finish_kernel(const long long *acc_all, uint32_t total, double inv_scale, double three_over_n, double *corr) {
  const uint32_t k = blockIdx.x * kClusterThreads + threadIdx.x;
  if (k < total) corr[k] += ((double)acc_all[k] * inv_scale) * three_over_n;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
template <class Geometry>
int sw_corr_update(const Geometry &g, const SwPlan &p, const SwWorkspace &ws, const SwRequest &r) {
  const uint32_t N = g.nvert(), B = r.B;
  const hipStream_t st = as_stream(r.stream);
  uint32_t *status = ws.status.in<uint32_t>(r.d_work), *count = ws.count.in<uint32_t>(r.d_work);
  unsigned long long *table = ws.table.in<unsigned long long>(r.d_work);
  long long *acc = ws.acc.in<long long>(r.d_work);
  const uint32_t *label = ws.label.in<uint32_t>(r.d_work);
  const long long *qa = ws.qa.in<long long>(r.d_work);
  MLMCPI_HIP_TRY(hipMemsetAsync(table, 0, ws.correlator_bytes(), st));
  hipLaunchKernelGGL(sigma_sw_slice_sum_kernel<Geometry>, dim3(B * p.resolve_blocks), dim3(kClusterThreads), 0, st, g, p.resolve_blocks, label,
                     qa, table, ws.lg, count, status);
  MLMCPI_LAUNCH_CHECK("sigma_sw_slice_sum_kernel");
  const uint32_t pair_blocks = ((1u << ws.lg) + kClusterThreads * kSwPairBatches - 1) / (kClusterThreads * kSwPairBatches);
  hipLaunchKernelGGL(sigma_sw_slice_pair_kernel, dim3(2 * B * pair_blocks), dim3(kClusterThreads), 0, st, (const unsigned long long *)table,
                     ws.lg, (const uint32_t *)count, N, g.extent(0), g.extent(1), pair_blocks, ldexp(1.0, (int)ws.s - 64), acc, status);
  MLMCPI_LAUNCH_CHECK("sigma_sw_slice_pair_kernel");
  const uint32_t total = B * ws.n_out;
  hipLaunchKernelGGL(sigma_sw_slice_finish_kernel, dim3((total + kClusterThreads - 1) / kClusterThreads), dim3(kClusterThreads), 0, st,
                     (const long long *)acc, total, ldexp(1.0, -(int)ws.s), 3.0 / (double)N, r.d_corr);
  MLMCPI_LAUNCH_CHECK("sigma_sw_slice_finish_kernel");
  return MLMCPI_OK;
}

template int sw_corr_update<LatticeGeometry>(const LatticeGeometry &, const SwPlan &, const SwWorkspace &, const SwRequest &);
template int sw_corr_update<RotatedGeometry>(const RotatedGeometry &, const SwPlan &, const SwWorkspace &, const SwRequest &);

}  // namespace mlmcpi
