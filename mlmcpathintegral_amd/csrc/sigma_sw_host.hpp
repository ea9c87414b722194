// sigma_sw_host.hpp -- what the host code of the Swendsen-Wang units calls of each other: the launch plan, the workspace
// layout and the request of a draw (sigma_sw.hip builds all three), and the few functions through which sigma_sw.hip has the
// kernels of sigma_sw_tiled.hip, sigma_sw_chain.hip and sigma_sw_correlator.hip launched.  A kernel is launched only by the
// unit that defines it.
#pragma once
#include "internal.hpp"

#include "sigma_cluster_device.hpp"

namespace mlmcpi {

struct SwPlan {
  bool ok, chain;
  uint32_t W, H, ntx, nty;                // tiled: tile extents (vertices; on a rotated level cells), tiles per direction
  uint32_t merge_blocks, resolve_blocks;  // tiled: workgroups per chain of launches 2 and 3
  size_t lds_bytes;                       // dynamic LDS of the chain kernel / of launch 1
};

// the plain draw, the draw with structure sums, the draw with the improved correlator: a workspace layout each, and an instance
// of the chain kernel each (on the geometry, on WithStructure, on WithRoots)
enum class SwFlavour { kPlain, kStructure, kCorrelator };

struct SwSection {
  size_t offset, bytes;
  template <class T>
  T *in(void *work) const { return (T *)((char *)work + offset); }
};

// The workspace of a draw, laid out once from (geometry, B, flavour) by sw_layout (sigma_sw.hip); every section is a multiple of
// 256 B, in this order:
//   status   the status word (256 B)
//   label    [B N] uint32
//   qa       [B N] int64, q(a)
//   sum      [B N] int64, the cluster sums
//   slots    structure only: four more [B N] int64 sections (slot k of a root is k sections behind its cluster sum)
//   bits     [B owners] uint8, the bond bits (two bits per vertex; on a rotated level four bits per E vertex)
//   table    correlator only, as are the two below: [B][2][2^lg] slots of 16 B, lg the smallest with 2^lg >= 2 N
//   count    [B][2][N] uint32, the occupied slices of a root
//   acc      [B][n_out] int64, the lag accumulators at the scale s (sw_lag_scale)
// table, count and acc are contiguous and cleared by one memset per update.  A section its flavour does not have is empty.
// The chain plan uses the status word only (with the correlator: label and qa as well); with structure sums it also keeps its
// table of weights, 16 (M_0 + M_1) B per chain, in `weights`, which is no section of its own: it lies over the int64 sections from
// qa on, which that plan does not use, and sw_layout checks that they hold it.
struct SwWorkspace {
  SwSection status, label, qa, sum, slots, bits, table, count, acc, weights;
  uint32_t lg, n_out, s;
  size_t bytes() const { return acc.offset + acc.bytes; }
  size_t slot_stride() const { return slots.bytes ? sum.bytes / sizeof(long long) : 0; }   // in int64; 0 without structure sums
  size_t correlator_bytes() const { return table.bytes + count.bytes + acc.bytes; }
};

// a draw as its entry point received it; the optional outputs may be NULL, d_structure and d_corr never both set
struct SwRequest {
  const char *what;                       // the entry point, for its messages
  double beta;
  double *d_phi;
  uint32_t B, n_updates;
  uint64_t seed;
  uint32_t chain0, update0;
  uint32_t *d_flipped, *d_clusters;
  double *d_improved, *d_structure, *d_corr;
  void *d_work, *stream;
};

// ---- sigma_sw_tiled.hip -------------------------------------------------------------------------------------------------------
// what the tiled plan asks of a geometry: the plane the tiles divide and the default tile, the crossing links of launch 2, the
// LDS of launch 1
void sw_tiling(const LatticeGeometry &g, uint32_t &pw, uint32_t &ph, uint32_t &W, uint32_t &H);
void sw_tiling(const RotatedGeometry &g, uint32_t &pw, uint32_t &ph, uint32_t &W, uint32_t &H);
uint32_t sw_crossing(const LatticeGeometry &g, const SwPlan &p);
uint32_t sw_crossing(const RotatedGeometry &g, const SwPlan &p);
size_t sw_tile_lds(const LatticeGeometry &g, uint32_t W, uint32_t H);
size_t sw_tile_lds(const RotatedGeometry &g, uint32_t W, uint32_t H);
int sw_tiled_init_attrs();
// the launches of one update of the tiled plan (bond + label, merge, resolve, and finish where outputs are asked for), the
// structure instances where r.d_structure is set; instantiated on LatticeGeometry and RotatedGeometry
template <class Geometry>
int sw_tiled_update(const Geometry &g, const SwPlan &p, const SwWorkspace &ws, const SwRequest &r, const RngKey &key);

// ---- sigma_sw_chain.hip -------------------------------------------------------------------------------------------------------
int sw_chain_init_attrs();
// one launch of the flavour's instance of the chain kernel: n_updates updates from `key` on; `name` is what a launch error shows
template <class Geometry>
int sw_chain_launch(const Geometry &g, SwFlavour flavour, const SwPlan &p, const SwWorkspace &ws, const SwRequest &r, uint32_t n_updates,
                    const RngKey &key, const char *name);

// ---- sigma_sw_correlator.hip --------------------------------------------------------------------------------------------------
// the three launches of the improved correlator for the update whose roots and q(a) the workspace holds
template <class Geometry>
int sw_corr_update(const Geometry &g, const SwPlan &p, const SwWorkspace &ws, const SwRequest &r);

}  // namespace mlmcpi
