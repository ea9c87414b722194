// sigma_smooth_host.hpp -- the driver of the smoothers of an O(3) sigma-model field, cooling (sigma_cooling.hip) and the gradient
// flow (sigma_flow.hip): the plan, the checks, the launch schedule and the run of a call are sigma_smooth.hip's, on the field of
// sigma_field.hip.  A smoother is its kernel and one Smoother that describes it; the units of a smoother's list are cooling sweeps
// or flow steps.  A kernel is launched only by the unit that defines it.  Includes sigma_level_device.hpp, so the including file is
// compiled without fp contraction.
#pragma once
#include "internal.hpp"

#include "sigma_level_device.hpp"

namespace mlmcpi {

struct SmoothPlan {
  uint32_t tw, th, nt, fuse, tiles_a, tiles;  // tile, workgroup size, units per launch at most; tiles along the plane's width, per chain
};

struct Smoother {
  const char *who, *adj, *item, *list;  // for the messages: "cooling" / "the flow", "cooling" / "flow", "depth" / "step count", "depths" / "steps"
  uint32_t max_items, max_count;        // entries of the list, the largest entry
  uint32_t Tuning::*knob[4];            // the option's tw, th, nt, fuse (0: the default)
  uint32_t dflt[4];
  size_t (*lds)(const SigmaLevel &L, const SmoothPlan &p, uint32_t K);  // LDS image of a launch of K fused units
  // [L.rot]: K units on every tile of every chain (`blocks` workgroups) from src to dst; eps: the flow's step size, cooling has none
  int (*launch[2])(const SigmaLevel &L, const SmoothPlan &p, uint32_t K, double eps, uint64_t blocks, const double *src, double *dst, hipStream_t st);
  const void *kernels[6];  // its instances: each may take the whole LDS, set once per device (`once`)
  DeviceOnce *once;
};

// What a call and its plan query refuse alike; the plan (one snapshot of the knobs per call) comes back through `plan`.  Its LDS
// image fits: the option table takes no plan whose images do not, the defaults' do, and the plan only shrinks tiles.
int smooth_check(const Smoother &s, const mlmcpi_sigma_level *level, uint32_t n_chains, const uint32_t *list, uint32_t n, SmoothPlan *plan);
// The units of every launch of a call, in order: at most p.fuse, never past the next listed point.  Returns the LDS image of the
// deepest launch (0 without a launch).
uint32_t smooth_schedule(const Smoother &s, const SigmaLevel &L, const SmoothPlan &p, const uint32_t *list, uint32_t n, uint8_t *launches,
                         uint32_t *n_launches);
int smooth_workspace_bytes(const Smoother &s, const mlmcpi_sigma_level *level, uint32_t n_chains, size_t *bytes);
// the call: stage, the scheduled launches between the two vector buffers, the measurement at each listed point, d_out's angles
int smooth_run(const Smoother &s, const mlmcpi_sigma_level *level, const double *d_state, uint32_t n_chains, double eps, const uint32_t *list,
               uint32_t n, double *d_q, double *d_chi, double *d_energy, double *d_out, void *d_work, size_t work_bytes, void *stream);

// the plan query into either public plan struct: the same fields, but for the name of the launch list
template <class Plan, size_t N>
int smooth_plan_query(const Smoother &s, const mlmcpi_sigma_level *level, uint32_t n_chains, const uint32_t *list, uint32_t n, Plan *plan,
                      uint8_t (Plan::*launches)[N]) {
  MLMCPI_REQUIRE(plan, "the %s plan query needs somewhere to write (plan is NULL)", s.adj);
  SmoothPlan p;
  if (int rc = smooth_check(s, level, n_chains, list, n, &p)) return rc;
  *plan = Plan{};
  plan->tw = p.tw;
  plan->th = p.th;
  plan->nt = p.nt;
  plan->fuse = p.fuse;
  plan->tiles = p.tiles;
  plan->n_measurements = n;
  plan->lds_bytes = smooth_schedule(s, make_level(*level), p, list, n, plan->*launches, &plan->n_launches);
  return MLMCPI_OK;
}

}  // namespace mlmcpi
