// lattice_sweep.hpp -- what the units of the 2-D sweep path share: lattice2d.hip (the launch plan and its executor),
// schwinger_sweeps.hip with schwinger_or_block.hip, gff_sweeps.hip and sigma2d.hip (each action's sweep kernels and their launcher).
// The device helpers both tile kernels use; the geometry the planner and the kernels agree on, each size defined once (what needs
// no sampler: sweep_geometry.hpp); and the launcher interface, one function per action.
#pragma once
#include "internal.hpp"
#include "site_update.hpp"
#include "step_envelope.hpp"
#include "sweep_geometry.hpp"
#include "vonmises.hpp"

namespace mlmcpi {

// ---- device helpers of the tile kernels ------------------------------------------------------------------------------------
// linear iteration of a workgroup over an nr x nc region without per-element division
template <int NT, class F>
__device__ __forceinline__ void for_region(uint32_t nr, uint32_t nc, F f) {
  const uint32_t total = nr * nc;
  uint32_t idx = threadIdx.x;
  if (idx >= total) return;
  uint32_t ri = idx / nc, ci = idx - ri * nc;
  uint32_t dr = NT / nc, dc = NT - dr * nc;
  for (; idx < total; idx += NT) {
    f(ri, ci);
    ri += dr;
    ci += dc;
    if (ci >= nc) {
      ci -= nc;
      ++ri;
    }
  }
}

// Staging loop for global -> LDS: the same traversal as for_region, but UNR independent loads are
// issued back to back before any of them is consumed, so a thread has UNR HBM requests in flight
// instead of one (a rolled load -> wait -> ds_write loop is latency bound: ~10 dependent round
// trips per tile).
template <int NT, int UNR, class T, class Load, class Store>
__device__ __forceinline__ void stage_region(uint32_t nr, uint32_t nc, Load load, Store store) {
  const uint32_t total = nr * nc;
  uint32_t idx = threadIdx.x;
  uint32_t ri = idx / nc, ci = idx - ri * nc;
  const uint32_t dr = NT / nc, dc = NT - dr * nc;
  while (idx < total) {
    T v[UNR];
    uint32_t rr[UNR], cc[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      rr[u] = ri;
      cc[u] = ci;
      if (idx + u * NT < total) v[u] = load(ri, ci);
      ri += dr;
      ci += dc;
      if (ci >= nc) {
        ci -= nc;
        ++ri;
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
      if (idx + u * NT < total) store(rr[u], cc[u], v[u]);
    idx += UNR * NT;
  }
}

__device__ __forceinline__ uint32_t wrap_add(uint32_t base, uint32_t off, uint32_t n) {
  uint32_t v = base + off;
  while (v >= n) v -= n;
  return v;
}

// ---- site-at-a-time updates: Action::heatbath_update / overrelaxation_update(state, l), action/action.hh:73-96 -----------
// gffaction.cc:33-42,68-77; quenchedschwingeraction.cc:25-65.  One thread per chain walks the site list in order (the
// reference's own sequential semantics: every update sees the ones before it), straight on the state in global memory.
// Same arithmetic and the same random numbers -- Philox (site, chain, step) -- as the sweep kernels, so the sites of a
// colour class visited in any order with the sweep's step reproduce that colour phase of the sweep.
// One template, two launching units: <false> belongs to lattice2d.hip (mlmcpi_lattice_site_updates), <true> to
// schwinger_sweeps.hip (schwinger_site_updates).  vs_exact_pair (step_envelope.hpp) is not inlined, and without relocatable
// device code the compiler specialises it for the callers it has in a unit: the Schwinger sweep kernels hand it the table in
// LDS, this kernel in global memory.  Only with both in one unit are the function and the sweep kernels generated as
// tools/kernel_digest.py records them (EXPERIMENTS.md 0.9).
template <bool SCHW>
__global__ void __launch_bounds__(64)
    lattice_site_update_kernel(uint32_t Mt, uint32_t Mx, double coupling, double *__restrict__ state, uint32_t B,
                               const uint32_t *__restrict__ sites, uint32_t n, uint32_t single, int heat, RngKey key0,
                               const uint32_t *__restrict__ vs_table) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  RngKey key = key0;
  key.chain += b;
  if (SCHW) {
    double *th = state + (size_t)b * 2 * Mt * Mx;
    const bool step = 2. * coupling <= kVsKappaMax;
    const VsTable tab = VsTable::in_global(vs_table);
    for (uint32_t q = 0; q < n; ++q) schwinger_site_update(th, Mt, Mx, sites ? sites[q] : single, heat != 0, step, coupling, key, tab);
  } else {
    double *phi = state + (size_t)b * Mt * Mx;
    const double inv_kappa = 1. / (4. + coupling), two_over_kappa = 2. / (4. + coupling), sigma = 1. / sqrt(4. + coupling);
    for (uint32_t q = 0; q < n; ++q)
      gff_site_update(phi, Mt, Mx, sites ? sites[q] : single, heat != 0, inv_kappa, two_over_kappa, sigma, key);
  }
}

// ---- geometry: the LDS sizes that depend on a sampler's list (the others: sweep_geometry.hpp) -----------------------------------
// LDS bytes in front of the tile image of a heat-bath launch of schwinger_sweep_kernel (kernel and host agree through this)
__host__ __device__ inline size_t sweep_pool_bytes(bool step, bool fixed, uint32_t cap) {
  const size_t b = step ? (fixed ? VsPool<uint16_t>::bytes(cap) : VsPool<uint32_t>::bytes(cap)) : HbPool::bytes(cap);
  return (b + 15) / 16 * 16;
}

// ---- Schwinger: the heat-bath sweep on an LDS image, behind the overrelaxation sweeps of the same launch ------------------
// A draw ends "... K overrelaxation sweeps, heat bath, QoI".  As two launches the state makes two round trips through HBM,
// and the two kernels leave opposite halves of the CU idle: the overrelaxation launch is bound by its load / store phases
// and the latencies of its colour phases, the heat bath by vector issue with its memory traffic hidden.  In one launch
// (schwinger_perm_heat_kernel) the workgroup that has just swept a tile K times lays the tile and the two rings the heat
// bath reads down as an LDS image, runs the heat-bath sweep of schwinger_sweep_kernel<true, ., 64, 32, true> on it
// (schwinger_image_heat) -- same regions (the pruned last-sweep form), same cells, same Philox words, same arithmetic:
// bit-identical results -- sums the QoI and writes the tile out.  One round trip instead of two, and the two workgroups of
// a CU are in different phases most of the time: the loads of one run under the sampler arithmetic of the other.
// This struct holds the sizes of that image (a 64 x 64 tile and two rings) and of the sampler's list in front of it.
struct HeatImageGeom {
  static constexpr int HB = 2, IW = 64 + 2 * HB, IH = 64 + 2 * HB;
  static constexpr size_t image_bytes = (size_t)2 * IW * IH * sizeof(double);
  // in front of the image: the sampler's tables and the list of open cells -- a colour phase leaves about 5 % of its ~2200
  // cells on it at beta = 1 (110 entries on average; a list that overflows leaves cells to their own lanes, measured at
  // +20 % on the launch with 64 entries)
  static constexpr uint32_t pool_cap = 544, hb_pool_cap = 128;   // step-envelope list (r05: 256 -> 544 for concentrations up to 16: a phase leaves up to a fifth of its ~2200 cells there); wrapped-Cauchy pool (24 B per entry)
  static constexpr size_t vs_pool_bytes = VsPool<uint32_t>::bytes(pool_cap), hb_pool_bytes = HbPool::bytes(hb_pool_cap);
  static constexpr size_t pool_bytes = ((vs_pool_bytes > hb_pool_bytes ? vs_pool_bytes : hb_pool_bytes) + 15) / 16 * 16;
  static constexpr size_t hb_bytes = image_bytes + pool_bytes;
  static_assert(image_bytes == 73984 && pool_bytes == 3424 && hb_bytes == 77408, "LDS layout of the fused launch");
  static_assert(hb_bytes <= OrBlockGeom<6>::lds_bytes, "two workgroups per CU");
};

// dynamic LDS of schwinger_perm_heat_kernel.  LDS: tables + list | the plane, then the image in the same place.
template <int NT, bool STEP>
struct PermHeatGeom {
  using PG = PermGeom<NT, 2>;
  using OH = HeatImageGeom;
  // (the packed plane of every depth is smaller than the image: one build, one LDS size)
  static constexpr size_t lds_bytes = OH::pool_bytes + (PG::plane_bytes > OH::image_bytes ? PG::plane_bytes : OH::image_bytes);
  static_assert(PG::plane_bytes <= OH::image_bytes, "the plane lies where the image follows it");
};

// ---- launchers: one SweepLaunch each --------------------------------------------------------------------------------
// The launch `l` of the action's draw: reads a.src, writes a.dst.  A launcher fetches what its kernels need (the sampler's table,
// the scratch for the QoI partials), launches the kernel and, where the launch carries the QoI, finishes it with one more launch.
// Kernels are launched only by the unit that defines them.
int schwinger_sweep_launch(const SweepLaunch &l, const SweepArgs &a);  // schwinger_sweeps.hip
int gff_sweep_launch(const SweepLaunch &l, const SweepArgs &a);        // gff_sweeps.hip
int sigma_sweep_launch(const SweepLaunch &l, const SweepArgs &a);      // sigma2d.hip
// The kernels of a unit whose LDS may exceed the 64 KiB default are allowed it, on the current device (init_sweep_kernels,
// lattice2d.hip, calls these once per device; the sigma model keeps its own once-per-device flag)
int schwinger_allow_lds();
int gff_allow_lds();
int sigma_init_sweep_kernels();
// the register blocks of the Schwinger model have a unit of their own (schwinger_or_block.hip): schwinger_sweep_launch passes
// their launches on to it, schwinger_allow_lds calls its share
int schwinger_or_block_launch(const SweepLaunch &l, const SweepArgs &a);
int schwinger_or_block_allow_lds();
// mlmcpi_lattice_site_updates for the Schwinger action (arguments checked there), as sigma_site_updates (internal.hpp)
int schwinger_site_updates(const mlmcpi_lattice_action *act, double *d_state, uint32_t B, const uint32_t *d_sites, uint32_t n,
                           uint32_t site, int32_t heat, uint64_t seed, uint32_t chain0, uint32_t step, hipStream_t st);

}  // namespace mlmcpi
