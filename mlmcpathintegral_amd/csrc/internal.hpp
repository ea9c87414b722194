// internal.hpp -- host-side plumbing shared by the translation units of libmlmcpi_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mlmcpi_hip.h"
#include "device_common.hpp"
#include "device_once.hpp"

namespace mlmcpi {

// error channel (thread local)
int fail(int status, const char *fmt, ...);
int fail_hip(hipError_t e, const char *what);

#define MLMCPI_HIP_TRY(expr)                              \
  do {                                                    \
    hipError_t e__ = (expr);                              \
    if (e__ != hipSuccess) return fail_hip(e__, #expr);   \
  } while (0)

// launch check: kernels report configuration errors through hipGetLastError
#define MLMCPI_LAUNCH_CHECK(name)                         \
  do {                                                    \
    hipError_t e__ = hipGetLastError();                   \
    if (e__ != hipSuccess) return fail_hip(e__, name);    \
  } while (0)

#define MLMCPI_REQUIRE(cond, ...)                         \
  do {                                                    \
    if (!(cond)) return fail(MLMCPI_ERR_INVALID, __VA_ARGS__); \
  } while (0)

inline hipStream_t as_stream(void *s) { return (hipStream_t)s; }

// init() once for the current device (device_once.hpp): what a unit's kernels need before their first launch there
template <class Init>
int once_per_device(DeviceOnce &once, Init init) {
  int dev = 0;
  MLMCPI_HIP_TRY(hipGetDevice(&dev));
  const int rc = device_once(once, dev, init);
  return rc == kDeviceOutOfRange ? fail(MLMCPI_ERR_INVALID, "device index %d out of range", dev) : rc;
}

// Library-owned scratch for reduction partials: one buffer per (host thread, device, stream), grown on demand (the
// first call of a given size allocates; steady state does not).  `stream` = the stream the caller launches on.
int scratch(size_t bytes, void **d_ptr, hipStream_t stream);

inline RngKey make_key(uint64_t seed, uint32_t chain0, uint32_t step) {
  return RngKey{(uint32_t)seed, (uint32_t)(seed >> 32), chain0, step};
}

// Tuning knobs (they never change results): read from the environment ONCE, at the first sweep call of the process, and
// settable afterwards through mlmcpi_set_option (tests flip them between calls).  A new knob is a field here and an entry in the
// table of options.hip.
struct Tuning {
  uint32_t tile_w = 0, tile_h = 0, tile_nt = 0;  // MLMCPI_SWEEP_TILE=TWxTHxNT (0: default geometry)
  bool or_block = false;                         // MLMCPI_OR_KERNEL=block: 4 x 4 register blocks sweep by sweep instead of the closed form (Schwinger)
  bool or_heat_split = false;                    // MLMCPI_OR_HEAT=split: the heat-bath sweep behind the last overrelaxation launch gets a launch of its own
  int or_heat_wide = 0;                          // MLMCPI_OR_HEAT=wide|narrow: 1024-thread workgroups for the fused launch (+1 / -1; 0: by the number of tiles)
  bool random_sweep_global = false;               // MLMCPI_RANDOM_SWEEP_HOME=global: the random-order sweep keeps the state in global memory whatever the lattice
  uint32_t random_sweep_chunk = 0;                // MLMCPI_RANDOM_SWEEP_CHUNK=k: rounds scheduled per pass of the random-order sweep (0: 254)
  int sigma_cluster_team = 0;                     // MLMCPI_SIGMA_CLUSTER_TEAM=wave|block: lanes that share a chain in the sigma-model Wolff update (1 / 2; 0: by the batch)
  bool sigma_cluster_map_global = false;          // MLMCPI_SIGMA_CLUSTER_BITMAP=global: its membership bitmap in the workspace whatever the lattice
  int sigma_sw_plan = 0;                          // MLMCPI_SIGMA_SW_PLAN=chain|tiled: launch plan of the sigma-model Swendsen-Wang update, sigma_sw.hip, lattice and rotated level (1 / 2; 0: by lattice and batch)
  uint32_t sigma_sw_tile_w = 0, sigma_sw_tile_h = 0;  // MLMCPI_SIGMA_SW_TILE=WxH: tile of its tiled plan, W, H in {8, 16, 32, 64} (0: 64x32 vertices; on a rotated level: 32x32 cells)
  uint32_t sigma_level_tw = 0, sigma_level_th = 0, sigma_level_nt = 0, sigma_level_fuse = 0;  // MLMCPI_SIGMA_LEVEL_PLAN=TWxTHxNTxK: rotated sigma sweep (0: 32x32x512x2)
  uint32_t sigma_cool_tw = 0, sigma_cool_th = 0, sigma_cool_nt = 0, sigma_cool_fuse = 0;  // MLMCPI_SIGMA_COOL_PLAN=TWxTHxNTxK: sigma cooling, plain and rotated levels (0: 32x32x512x2)
  uint32_t sigma_flow_tw = 0, sigma_flow_th = 0, sigma_flow_nt = 0, sigma_flow_fuse = 0;  // MLMCPI_SIGMA_FLOW_PLAN=TWxTHxNTxK: sigma gradient flow, plain and rotated levels (0: 16x16x512x1)
  uint32_t sigma_twolevel_groups = 0;            // MLMCPI_SIGMA_TWOLEVEL_GROUPS=g: groups of 256 vertices per workgroup of the sigma two-level pass (0: 1)
};
Tuning tuning();  // a copy taken under the lock: callers snapshot it once per call

// Table of the step-envelope heat-bath sampler for an action of the given scale (2 beta, 2 m0 / a), in the memory of the
// current device: built and uploaded on first use (step_envelope.hpp, step_envelope_tables.hip).
int vs_table_device(double scale, const uint32_t **d_table);

// the O(3) nonlinear sigma model (sigma2d.hip); arguments checked by the lattice entry points that dispatch here
int sigma_evaluate(const mlmcpi_lattice_action *act, const double *d_phi, uint32_t B, double *d_S, hipStream_t st);
int sigma_force(const mlmcpi_lattice_action *act, const double *d_phi, double *d_f, uint32_t B, hipStream_t st);
int sigma_initialise(const mlmcpi_lattice_action *act, double *d_phi, uint32_t B, uint64_t seed, uint32_t chain0, hipStream_t st);
int sigma_site_updates(const mlmcpi_lattice_action *act, double *d_state, uint32_t B, const uint32_t *d_sites, uint32_t n,
                       uint32_t site, int32_t heat, uint64_t seed, uint32_t chain0, uint32_t step, hipStream_t st);
constexpr uint32_t kSigmaLdsMax = 160 * 1024 - 512;  // dynamic LDS a workgroup of sigma_sweep_kernel may take (static: the 3 x NT/64 reduction)

inline double gff_mu2(const mlmcpi_lattice_action &A) {  // gffaction.hh:174-181 (unrotated lattice)
  const double a_lat = 1. / A.Mt;
  return a_lat * a_lat * A.mass * A.mass;
}

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }  // workspace sections
// workgroups of 256 threads in x for a grid-stride loop over n entries (y: the chains)
inline uint32_t stream_blocks(size_t n) { return n > 1024 * 256 ? 1024u : (uint32_t)((n + 255) / 256); }

// ---- GFF and Schwinger on the 2-D lattice: what the translation units of lattice2d.hip's family call in each other.
// Kernels are launched only by the unit that defines them.
// lattice_reduce.hip
int check_lattice(const mlmcpi_lattice_action *act, bool square_gff = true);  // square_gff: the GFF action's own demand, Mt == Mx
int refuse_sigma(const mlmcpi_lattice_action *act, const char *what);          // the entry points the O(3) sigma model does not take
uint32_t row_blocks(uint32_t Mx, uint32_t B);                                  // workgroups per chain of the kernels that stride over rows
int lattice_energy(const mlmcpi_lattice_action *act, const double *d_phi, uint32_t B, double *d_S, hipStream_t st);
// d_out[b] = scale * sum of the squares of the n entries of chain b
int lattice_sum_squares(const double *d_x, uint32_t n, uint32_t B, double scale, double *d_out, hipStream_t st);
// partial[b * tiles + t] summed over t in a fixed order -> d_out[b] (op L_CHARGE: its square / 4 pi^2; else scale * sum);
// d_acc != NULL: the value recorded there as well (mlmcpi_stats_accumulate's sums)
int lattice_finish(const double *partial, uint32_t tiles, uint32_t B, int op, double scale, double *d_out, double *d_acc, hipStream_t st);
// gff_exact.hip: GFFAction::initialise_state, the exact sampler on the library's scratch
int gff_initialise_exact(const mlmcpi_lattice_action *act, double *d_phi, uint32_t B, uint64_t seed, uint32_t chain0, hipStream_t st);

constexpr uint32_t kComputeUnits = 256;  // MI355X
constexpr uint32_t kMaxFuse = 16;  // max sweeps fused in one launch (kinds travel in a bitmask)

}  // namespace mlmcpi
