// sigma_sw_chain.hip -- the chain plan of the Swendsen-Wang update of the O(3) nonlinear sigma model (sigma_sw.hip has the
// update, the RNG contract and the plan that chooses between this and the tiled plan of sigma_sw_tiled.hip): one workgroup per
// chain, all updates of a call in one launch.  One kernel, instantiated on the two geometries of sigma_cluster_device.hpp and,
// for the draws with structure sums and with the improved correlator, on WithStructure and WithRoots of either
// (sigma_sw_device.hpp); the estimators are described in sigma_sw_tiled.hip and sigma_sw_correlator.hip, and the chain kernel
// gives their bits.
#include <type_traits>

#include "sigma_sw_host.hpp"

#include "sigma_sw_device.hpp"  // fp contraction is off from here on

namespace mlmcpi {

// ---- chain plan: one workgroup per chain, all n_updates updates in one launch, labels, sums and a in LDS ------------------
// Thread t owns the vertices t, t + 1024, ..: it alone reads and writes their angles, update after update.  Bonds are drawn and
// united from the vertices that own links: every vertex its +i and +j link on the lattice; on a rotated level a lane with an E
// vertex makes two Philox calls and handles its four links, a lane with an O vertex makes none.
template <class Geometry>
__global__ void __launch_bounds__(kClusterBlockThreads)
    sigma_sw_chain_kernel(double2 *phi_all, Geometry g, double beta2, uint32_t n_updates, RngKey key0, uint32_t *flipped,
                          uint32_t *clusters, double *improved, uint32_t *status) {
  extern __shared__ double sw_lds[];
  __shared__ double red[kClusterBlockThreads];
  __shared__ uint32_t redc[kClusterBlockThreads];
  constexpr uint32_t NL = Geometry::kOwnedLinks;
  const uint32_t N = g.nvert(), owners = g.nowners(), b = blockIdx.x, t = threadIdx.x;
  double *a = sw_lds;
  long long *sum = (long long *)(a + N);
  uint32_t *parent = (uint32_t *)(sum + N);
  double2 *phi = phi_all + (size_t)b * N;
  const bool outputs = clusters || improved;
  RngKey key = key0;
  key.chain = key0.chain + b;
  uint32_t nflip = 0;
  bool capped = false;
  if constexpr (Geometry::kStructure) {
    // the weights of every position of both directions, once per launch, into this chain's table in the workspace: (cos, sin)
    // of position x of direction d at 2 (d M_0 + x).  Formed by sw_phase as everywhere; inside the update loop sincospi would
    // take the kernel beyond its 128 registers.  The barrier of the first update orders the table before its readers.
    const uint32_t M0 = g.extent(0), M1 = g.extent(1);
    double *table = g.weights + (size_t)b * 2 * (M0 + M1);
    for (uint32_t x = t; x < M0 + M1; x += kClusterBlockThreads) {
      const uint32_t d = x >= M0 ? 1u : 0u;
      double ws, wc;
      sw_phase(x - d * M0, d ? M1 : M0, ws, wc);
      table[2 * x] = wc;
      table[2 * x + 1] = ws;
    }
  }
  for (uint32_t n = 0; n < n_updates; ++n, ++key.step) {
    const V3 r = reflection_normal(key, P_SIGMA_SW_REFLECT);
    for (uint32_t l = t; l < N; l += kClusterBlockThreads) {
      a[l] = dot3(r, sigma_of(phi[l]));
      sum[l] = 0;
      parent[l] = l;
    }
    __syncthreads();
    for (uint32_t l = t; l < owners; l += kClusterBlockThreads) {
      uint32_t y[NL];
      g.far_ends(l, y);
      double ay[NL];
#pragma unroll
      for (uint32_t d = 0; d < NL; ++d) ay[d] = a[y[d]];
      const uint32_t bits = Geometry::bonds(key, l, a[l], ay, beta2);
#pragma unroll
      for (uint32_t d = 0; d < NL; ++d)
        if (bits & (1u << d)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, l, y[d], N, capped);
    }
    __syncthreads();
    for (uint32_t l = t; l < N; l += kClusterBlockThreads) {
      // structure instance: the root is stored over the parent (a lane that reads the word meanwhile gets the old parent or the
      // root, both above it), so that the four passes below read it in one load.  A root stores itself over itself and no other
      // vertex can come to hold its own index, so parent[l] == l holds for the same l as before: sw_finish sees the same roots
      // and the same sums as the plain instance, and d_improved and d_clusters are its bits.
      const uint32_t root = uf_find<Geometry::kStructure ? __HIP_MEMORY_SCOPE_WORKGROUP : kUfPlain>(parent, l, N, capped);
      if constexpr (Geometry::kStructure) __hip_atomic_store(parent + l, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if constexpr (Geometry::kRoots) {                    // the improved correlator reads both from the workspace
        g.roots[(size_t)b * N + l] = root;
        g.qa[(size_t)b * N + l] = sw_fixed(a[l]);
      }
      if (improved) atomicAdd((unsigned long long *)(sum + root), (unsigned long long)sw_fixed(a[l]));
      if (!capped && sw_coin(key, root)) {
        phi[l] = reflected(sigma_of(phi[l]), a[l], r);
        ++nflip;
      }
    }
    __syncthreads();
    if constexpr (!Geometry::kStructure) {
      if (outputs) sw_finish(parent, sum, N, red, redc, improved ? improved + b : nullptr, clusters ? clusters + b : nullptr);
      __syncthreads();
    } else {
      // Pass 0 finishes the cluster sums as above.  Pass k = 1 + 2 d + (0: cos, 1: sin) takes the one slot per vertex again: zero,
      // add q(a w) onto the root's slot, finish into structure[b][d].  a is still the field's before the update, w comes from the
      // table; the trip counts are uniform (sw_add_combined shuffles).  One copy of the code serves the five passes.
      const double *table = g.weights + (size_t)b * 2 * (g.extent(0) + g.extent(1));
#pragma unroll 1
      for (uint32_t k = 0; k < 5; ++k) {
        const uint32_t d = k ? (k - 1) >> 1 : 0;
        if (k > 0) {
          for (uint32_t l = t; l < N; l += kClusterBlockThreads) sum[l] = 0;
          __syncthreads();
#pragma unroll 1
          for (uint32_t base = 0; base < N; base += kClusterBlockThreads) {
            const uint32_t l = base + t;
            const bool active = l < N;
            const long long v[1] = {active ? sw_fixed(a[l] * table[2 * (d * g.extent(0) + g.position(l, d)) + ((k - 1) & 1u)]) : 0};
            sw_add_combined<__HIP_MEMORY_SCOPE_WORKGROUP>(sum, 0, active ? parent[l] : 0u, active, v);
          }
          __syncthreads();
        }
        if (k > 0 || outputs)
          sw_finish(parent, sum, N, red, redc, k ? g.structure + 2 * b + d : (improved ? improved + b : nullptr),
                    k || !clusters ? nullptr : clusters + b);
        __syncthreads();
      }
    }
  }
  if (flipped) {
    for (int off = kWave / 2; off > 0; off >>= 1) nflip += __shfl_down(nflip, off);
    if ((t & (kWave - 1)) == 0 && nflip) atomicAdd(flipped + b, nflip);
  }
  if (capped) atomicOr(status, 1u);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// dynamic LDS above 64 KiB: every instance up to the plan's bound
int sw_chain_init_attrs() {
  const void *const instances[] = {(const void *)sigma_sw_chain_kernel<LatticeGeometry>,
                                   (const void *)sigma_sw_chain_kernel<RotatedGeometry>,
                                   (const void *)sigma_sw_chain_kernel<WithStructure<LatticeGeometry>>,
                                   (const void *)sigma_sw_chain_kernel<WithStructure<RotatedGeometry>>,
                                   (const void *)sigma_sw_chain_kernel<WithRoots<LatticeGeometry>>,
                                   (const void *)sigma_sw_chain_kernel<WithRoots<RotatedGeometry>>};
  for (const void *kernel : instances)
    MLMCPI_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSwChainMaxN * kSwChainBytesPerVertex));
  return MLMCPI_OK;
}

// kStructure: the instance forms its weights in the workspace (ws.weights) and adds to r.d_structure.  kCorrelator: the
// instance leaves the roots and q(a) where the tiled plan has them (ws.label, ws.qa); the caller asks for one update per launch.
template <class Geometry>
int sw_chain_launch(const Geometry &g, SwFlavour flavour, const SwPlan &p, const SwWorkspace &ws, const SwRequest &r, uint32_t n_updates,
                    const RngKey &key, const char *name) {
  const auto launch = [&](const auto &instance) {
    using Instance = std::decay_t<decltype(instance)>;
    hipLaunchKernelGGL(sigma_sw_chain_kernel<Instance>, dim3(r.B), dim3(kClusterBlockThreads), p.lds_bytes, as_stream(r.stream),
                       (double2 *)r.d_phi, instance, 2.0 * r.beta, n_updates, key, r.d_flipped, r.d_clusters, r.d_improved,
                       ws.status.in<uint32_t>(r.d_work));
    MLMCPI_LAUNCH_CHECK(name);
    return (int)MLMCPI_OK;
  };
  switch (flavour) {
    case SwFlavour::kStructure: return launch(WithStructure<Geometry>(g, r.d_structure, ws.weights.in<double>(r.d_work)));
    case SwFlavour::kCorrelator: return launch(WithRoots<Geometry>(g, ws.label.in<uint32_t>(r.d_work), ws.qa.in<long long>(r.d_work)));
    default: return launch(g);
  }
}

template int sw_chain_launch<LatticeGeometry>(const LatticeGeometry &, SwFlavour, const SwPlan &, const SwWorkspace &, const SwRequest &,
                                              uint32_t, const RngKey &, const char *);
template int sw_chain_launch<RotatedGeometry>(const RotatedGeometry &, SwFlavour, const SwPlan &, const SwWorkspace &, const SwRequest &,
                                              uint32_t, const RngKey &, const char *);

}  // namespace mlmcpi
