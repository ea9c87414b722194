// sigma_field_device.hpp -- a field of unit vectors of the O(3) sigma model in a caller's workspace, and what is measured on it.
// sigma_field.hip defines everything declared here and owns the kernels; the smoothing driver (sigma_smooth.hip) calls it, the
// smoothers (sigma_cooling.hip, sigma_flow.hip) use the accessors in their kernels.  Per chain three planes x[n], y[n], z[n] in the
// level's vertex order.  Includes sigma_topology_device.hpp, so the including file is compiled without fp contraction.
#pragma once
#include "sigma_topology_device.hpp"

namespace mlmcpi {

// vertex l of a chain's buffer v[3][n]
__device__ __forceinline__ V3 field_fetch(const double *v, uint32_t n, size_t l) { return V3{v[l], v[n + l], v[2 * (size_t)n + l]}; }

__device__ __forceinline__ void field_store(double *v, uint32_t n, size_t l, const V3 &s) {
  v[l] = s.x;
  v[n + l] = s.y;
  v[2 * (size_t)n + l] = s.z;
}

// The workspace of a call: two vector buffers (ping-pong), the charge partials (one per 32 x 32 tile and chain) and the energy
// partials (one per group of 256 vertices and chain), in this order.
struct FieldWork {
  size_t vec, part_q, part_e, total;  // bytes of one vector buffer, of the charge partials, of the energy partials
  uint32_t ngroups;
};
FieldWork field_work(const SigmaLevel &L, uint32_t n_chains);

// the sections of a workspace d_work
struct FieldBuffers { double *cur, *other, *part_q, *part_e; };
inline FieldBuffers field_carve(const FieldWork &w, void *d_work) {
  char *p = (char *)d_work;
  return FieldBuffers{(double *)p, (double *)(p + w.vec), (double *)(p + 2 * w.vec), (double *)(p + 2 * w.vec + w.part_q)};
}

// The launches below make n_chains * ngroups workgroups each, the charge launch n_chains * topo_plan(L).tiles.
// sigma_field_stage_kernel: sigma_of(angles) of every chain of d_state -> vec
int field_stage(const SigmaLevel &L, const FieldWork &w, uint32_t n_chains, const double *d_state, double *vec, hipStream_t st);
// sigma_field_charge_kernel, sigma_field_energy_kernel (each only where its outputs are asked for) and sigma_field_finish_kernel on
// the field `vec`: column k of the outputs [n_chains][n_cols]
int field_measure(const SigmaLevel &L, const FieldWork &w, uint32_t n_chains, const double *vec, double *part_q, double *part_e,
                  uint32_t n_cols, uint32_t k, double *d_q, double *d_chi, double *d_energy, hipStream_t st);
// sigma_field_angles_kernel: the angles of the field `vec` -> d_out [n_chains][2 n]
int field_angles(const SigmaLevel &L, const FieldWork &w, uint32_t n_chains, const double *vec, double *d_out, hipStream_t st);

}  // namespace mlmcpi
