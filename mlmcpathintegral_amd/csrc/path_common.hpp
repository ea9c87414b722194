// path_common.hpp -- what the translation units of the 1-D paths (harmonic / quartic oscillator, topological rotor; B chains
// laid out chain-major x[b*M + j]) share: the action's parameters, the three site formulas, and the host functions the units
// call in each other.  Kernels are launched only by the unit that defines them.
//   path1d.hip         evaluate / force / initialise, the QoI reductions, fine <-> coarse copies
//   path_hmc.hip       fused HMC: one trajectory per launch, or whole chains in one launch
//   rotor_sweeps.hip   the rotor's overrelaxation / heat-bath sweeps on LDS-resident segments, site-at-a-time updates
//   path_twolevel.hip  the two-level Metropolis step
//   ho_exact.hip       exact sampler of the harmonic oscillator
#pragma once
#include <type_traits>

#include "internal.hpp"

namespace mlmcpi {

struct PathP {
  int kind;
  uint32_t M;
  double a, m0, mu2, lambda, x0;
  double c1;      // m0 / a
  double c2;      // 2 + a^2 mu2
  double c3;      // a lambda
  double inv_a2;  // 1 / a^2
  double T_final;
};

inline PathP make_params(const mlmcpi_path_action &A) {
  PathP P;
  P.kind = A.kind;
  P.M = A.M;
  P.T_final = A.T_final;
  P.a = A.T_final / A.M;  // lattice/lattice1d.cc:9
  P.m0 = A.m0;
  P.mu2 = A.mu2;
  P.lambda = A.lambda;
  P.x0 = A.x0;
  P.c1 = A.m0 / P.a;
  P.c2 = 2. + P.a * P.a * A.mu2;
  P.c3 = P.a * A.lambda;
  P.inv_a2 = 1. / (P.a * P.a);
  return P;
}

// Site term of the action involving x_j and its left neighbour; S = energy_scale * sum_j term_j.
//   HO       harmonicoscillatoraction.cc:8-18     S = (a m0/2) sum [ (dx)^2/a^2 + mu2 x^2 ]
//   quartic  quarticoscillatoraction.cc:7-27      S = (a/2) sum [ m0((dx)^2/a^2 + mu2 x^2) + (lambda/2)(x-x0)^4 ]
//   rotor    rotoraction.cc:9-18                  S = (m0/a) sum [ 1 - cos(dx) ]
template <int KIND>
__device__ __forceinline__ double site_energy(const PathP &P, double x, double xl) {
  const double d = x - xl;
  if (KIND == MLMCPI_HARMONIC) return P.inv_a2 * d * d + P.mu2 * x * x;
  if (KIND == MLMCPI_QUARTIC) {
    const double sh = x - P.x0, sh2 = sh * sh;
    return P.m0 * (P.inv_a2 * d * d + P.mu2 * (x * x)) + 0.5 * P.lambda * sh2 * sh2;
  }
  return 1. - cos(d);
}

__host__ __device__ inline double energy_scale(const PathP &P) {
  if (P.kind == MLMCPI_HARMONIC) return 0.5 * P.a * P.m0;
  if (P.kind == MLMCPI_QUARTIC) return 0.5 * P.a;
  return P.m0 / P.a;
}

// Force on site j.  HO harmonicoscillatoraction.cc:21-35, quartic quarticoscillatoraction.cc:30-53,
// rotor rotoraction.cc:59-79.
template <int KIND>
__device__ __forceinline__ double site_force(const PathP &P, double xl, double x, double xr) {
  if (KIND == MLMCPI_ROTOR) return P.c1 * (sin(x - xl) + sin(x - xr));
  double f = P.c1 * (P.c2 * x - xl - xr);
  if (KIND == MLMCPI_QUARTIC) {
    const double sh = x - P.x0;
    f += P.c3 * sh * sh * sh;
  }
  return f;
}

// f(std::integral_constant<int, KIND>{}) for the action's kind; the entry points have checked it (check_action)
template <class F>
inline auto dispatch_kind(int kind, F &&f) {
  switch (kind) {
    case MLMCPI_HARMONIC: return f(std::integral_constant<int, MLMCPI_HARMONIC>{});
    case MLMCPI_QUARTIC: return f(std::integral_constant<int, MLMCPI_QUARTIC>{});
    default: return f(std::integral_constant<int, MLMCPI_ROTOR>{});
  }
}

enum ReduceOp { R_ENERGY = 0, R_XSQUARED = 1, R_WINDING = 2 };

// path1d.hip
int check_action(const mlmcpi_path_action *act);
uint32_t choose_split(uint32_t sites, uint32_t B);  // workgroups per chain of the kernels that stride over sites
// d_out[b] = finish(sum over the sites of chain b of the site term of `op`), on the library's scratch
int path_reduce(int op, const PathP &P, const double *d_x, uint32_t B, double scale, double *d_out, hipStream_t st);
// partial[b * nsplit + s] summed over s in a fixed order -> d_out[b] (op R_WINDING: its square / 4 pi^2 times scale; else
// scale * sum); d_acc != NULL: the value recorded there as well (mlmcpi_stats_accumulate's sums)
int path_finish(const double *partial, uint32_t nsplit, uint32_t B, int op, double scale, double *d_out, double *d_acc, hipStream_t st);

}  // namespace mlmcpi
