// lattice_twolevel.hip -- what couples two levels of the Schwinger / GFF lattice hierarchy: the transfers between a
// fine and a coarse lattice, and the two-level Metropolis step with its conditioned fine actions.
#include <cmath>
#include <mutex>

#include "fillin.hpp"
#include "internal.hpp"
#include "vonmises.hpp"

// =================================================================================================
// Transfers between lattice levels: Action::copy_from_fine / copy_from_coarse for the 2-D actions.
//   Schwinger  quenchedschwingeraction.cc:92-195 (three coarsening cases: both, temporal, spatial)
//   GFF        gffaction.cc:97-118 (fine2coarse_map of lattice2d.cc:126-134; unrotated coarsenings)
// Grid (rows, B); rt, rx in {1, 2} are the coarsening factors in the temporal / spatial direction.
// =================================================================================================
namespace mlmcpi {

__global__ void __launch_bounds__(256)
    schwinger_copy_from_fine_kernel(uint32_t Mt, uint32_t Mx, uint32_t rt, uint32_t rx, const double2 *__restrict__ fine_all,
                                    double2 *__restrict__ coarse_all) {
  const uint32_t b = blockIdx.y, Mtf = Mt * rt, Mxf = Mx * rx;  // Mt, Mx: coarse extents
  const double2 *fine = fine_all + (size_t)b * Mtf * Mxf;
  double2 *coarse = coarse_all + (size_t)b * Mt * Mx;
  for (uint32_t j = blockIdx.x; j < Mx; j += gridDim.x)
    for (uint32_t i = threadIdx.x; i < Mt; i += blockDim.x) {
      const size_t f = (size_t)(rx * j) * Mtf + rt * i;
      // mu = 0 links add up along the temporal direction, mu = 1 links along the spatial one
      const double t0 = (rt == 2) ? fine[f].x + fine[f + 1].x : fine[f].x;
      const double t1 = (rx == 2) ? fine[f].y + fine[f + Mtf].y : fine[f].y;
      coarse[(size_t)j * Mt + i] = make_double2(mod_2pi(t0), mod_2pi(t1));
    }
}

// writes only the links the reference writes (the others are filled by the conditioned fine action)
__global__ void __launch_bounds__(256)
    schwinger_copy_from_coarse_kernel(uint32_t Mt, uint32_t Mx, uint32_t rt, uint32_t rx,
                                      const double2 *__restrict__ coarse_all, double *__restrict__ fine_all) {
  const uint32_t b = blockIdx.y, Mtf = Mt * rt, Mxf = Mx * rx;
  const double2 *coarse = coarse_all + (size_t)b * Mt * Mx;
  double *fine = fine_all + (size_t)b * 2 * Mtf * Mxf;
  for (uint32_t j = blockIdx.x; j < Mx; j += gridDim.x)
    for (uint32_t i = threadIdx.x; i < Mt; i += blockDim.x) {
      const double2 c = coarse[(size_t)j * Mt + i];
      const size_t f = 2 * ((size_t)(rx * j) * Mtf + rt * i);  // link index of (rt i, rx j, 0)
      if (rt == 2) {
        fine[f] = 0.5 * c.x;
        fine[f + 2] = 0.5 * c.x;
      } else {
        fine[f] = c.x;
      }
      if (rx == 2) {
        fine[f + 1] = 0.5 * c.y;
        fine[f + 2 * Mtf + 1] = 0.5 * c.y;
      } else {
        fine[f + 1] = c.y;
      }
    }
}

// to_coarse != 0: coarse(i,j) = fine(rt i, rx j); else fine(rt i, rx j) = coarse(i,j)
__global__ void __launch_bounds__(256)
    vertex_transfer_kernel(uint32_t Mt, uint32_t Mx, uint32_t rt, uint32_t rx, double *__restrict__ fine_all,
                           double *__restrict__ coarse_all, int to_coarse) {
  const uint32_t b = blockIdx.y, Mtf = Mt * rt, Mxf = Mx * rx;
  double *fine = fine_all + (size_t)b * Mtf * Mxf, *coarse = coarse_all + (size_t)b * Mt * Mx;
  for (uint32_t j = blockIdx.x; j < Mx; j += gridDim.x)
    for (uint32_t i = threadIdx.x; i < Mt; i += blockDim.x) {
      const size_t f = (size_t)(rx * j) * Mtf + rt * i, c = (size_t)j * Mt + i;
      if (to_coarse) coarse[c] = fine[f]; else fine[f] = coarse[c];
    }
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

static int check_levels(const mlmcpi_lattice_action *fine, uint32_t rt, uint32_t rx) {
  if (int rc = check_lattice(fine, false)) return rc;
  if (int rc = refuse_sigma(fine, "copying between levels")) return rc;
  if (!((rt == 1 || rt == 2) && (rx == 1 || rx == 2) && rt * rx > 1))
    return fail(MLMCPI_ERR_INVALID, "cannot copy between these lattices (coarsening factors %u x %u)", rt, rx);
  if (fine->Mt % rt || fine->Mx % rx) return fail(MLMCPI_ERR_INVALID, "fine lattice %u x %u cannot be coarsened by %u x %u", fine->Mt, fine->Mx, rt, rx);
  return MLMCPI_OK;
}

int mlmcpi_lattice_copy_from_fine(const mlmcpi_lattice_action *fine, uint32_t rt, uint32_t rx, const double *d_fine,
                                  double *d_coarse, uint32_t B, void *stream) {
  if (int rc = check_levels(fine, rt, rx)) return rc;
  MLMCPI_REQUIRE(d_fine && d_coarse && B > 0, "bad arguments");
  const uint32_t Mt = fine->Mt / rt, Mx = fine->Mx / rx;
  dim3 grid(row_blocks(Mx, B), B), block(256);
  if (fine->kind == MLMCPI_SCHWINGER)
    hipLaunchKernelGGL(schwinger_copy_from_fine_kernel, grid, block, 0, as_stream(stream), Mt, Mx, rt, rx,
                       (const double2 *)d_fine, (double2 *)d_coarse);
  else
    hipLaunchKernelGGL(vertex_transfer_kernel, grid, block, 0, as_stream(stream), Mt, Mx, rt, rx, (double *)d_fine, d_coarse, 1);
  MLMCPI_LAUNCH_CHECK("copy_from_fine kernel");
  return MLMCPI_OK;
}

int mlmcpi_lattice_copy_from_coarse(const mlmcpi_lattice_action *fine, uint32_t rt, uint32_t rx, const double *d_coarse,
                                    double *d_fine, uint32_t B, void *stream) {
  if (int rc = check_levels(fine, rt, rx)) return rc;
  MLMCPI_REQUIRE(d_fine && d_coarse && B > 0, "bad arguments");
  const uint32_t Mt = fine->Mt / rt, Mx = fine->Mx / rx;
  dim3 grid(row_blocks(Mx, B), B), block(256);
  if (fine->kind == MLMCPI_SCHWINGER)
    hipLaunchKernelGGL(schwinger_copy_from_coarse_kernel, grid, block, 0, as_stream(stream), Mt, Mx, rt, rx,
                       (const double2 *)d_coarse, d_fine);
  else
    hipLaunchKernelGGL(vertex_transfer_kernel, grid, block, 0, as_stream(stream), Mt, Mx, rt, rx, d_fine, (double *)d_coarse, 0);
  MLMCPI_LAUNCH_CHECK("copy_from_coarse kernel");
  return MLMCPI_OK;
}

}  // extern "C"

// =================================================================================================
// Two-level Metropolis step on the Schwinger lattice with semi-coarsening (one direction halved):
//   TwoLevelMetropolisStep::draw                               montecarlo/twolevelmetropolisstep.cc:35-89
//   QuenchedSchwingerAction::copy_from_{coarse,fine}           action/qft/quenchedschwingeraction.cc:92-195
//   QuenchedSchwingerSemiConditionedFineAction::{fill_fine_points,evaluate}
//                                                              action/qft/quenchedschwingerconditionedfineaction.cc:130-204,332-379
// One coarse cell (i, j) owns two fine vertices.  In the coarsened direction d the coarse link splits into a
// pair  a0 = theta_c/2 + dtheta, a1 = theta_c/2 - dtheta  (dtheta ~ U(-pi, pi)); the coarse link in the other
// direction is copied; the remaining fine link (direction 1-d, between the two halves) is drawn from its
// heat-bath conditional (ExpCos) given the staples  theta_p = s0 + b0 - a0,  theta_m = a1 + s2 - b1, where
// (b0, b1) is the pair of the neighbouring cell and s2 the copied link of the next cell.  The neighbour's pair
// is recomputed from its own Philox stream (no exchange).  RNG: dtheta of coarse cell c = Philox(site c,
// P_FILLIN, 0); the ExpCos draw of fine link l = von Mises stream (site l, kVmFillin).
// =================================================================================================
namespace mlmcpi {

// theta (fine, double2 per vertex) in reference order; rt = 2: temporal coarsening, else spatial (rx = 2).
// partial[(b * gridDim.x + blockIdx.x) * 2 + {0, 1}] = CFA sums of (theta', theta).
__global__ void __launch_bounds__(256)
    schwinger_twolevel_propose_kernel(uint32_t Mtc, uint32_t Mxc, uint32_t rt, double beta,
                                      const double2 *__restrict__ coarse_all, const double2 *__restrict__ theta_all,
                                      double2 *__restrict__ prime_all, double *__restrict__ partial, RngKey key0) {
  __shared__ double red[2 * 4];
  const uint32_t b = blockIdx.y;
  const uint32_t Mtf = (rt == 2) ? 2 * Mtc : Mtc, Mxf = (rt == 2) ? Mxc : 2 * Mxc;
  const double2 *coarse = coarse_all + (size_t)b * Mtc * Mxc;
  const double2 *theta = theta_all + (size_t)b * Mtf * Mxf;
  double2 *prime = prime_all + (size_t)b * Mtf * Mxf;
  RngKey key = key0;
  key.chain += b;
  double acc[2] = {0.0, 0.0};
  for (uint32_t j = blockIdx.x; j < Mxc; j += gridDim.x) {
    const uint32_t jp = j + 1 == Mxc ? 0 : j + 1;
    for (uint32_t i = threadIdx.x; i < Mtc; i += blockDim.x) {
      const uint32_t ip = i + 1 == Mtc ? 0 : i + 1;
      const uint32_t c = j * Mtc + i;
      // neighbour cell in the direction the pair does NOT point in, and the next cell along the pair
      const uint32_t cn = (rt == 2) ? jp * Mtc + i : j * Mtc + ip;
      const uint32_t cs = (rt == 2) ? j * Mtc + ip : jp * Mtc + i;
      const double2 lc = coarse[c], ln = coarse[cn], ls = coarse[cs];
      const double pair_c = (rt == 2) ? lc.x : lc.y, pair_n = (rt == 2) ? ln.x : ln.y;
      const double s0 = (rt == 2) ? lc.y : lc.x, s2 = (rt == 2) ? ls.y : ls.x;
      double u, v;
      rng_uniforms(key, c, P_FILLIN, 0, u, v);
      const double d_c = (2. * u - 1.) * kPi;
      rng_uniforms(key, cn, P_FILLIN, 0, u, v);
      const double d_n = (2. * u - 1.) * kPi;
      const double a0 = mod_2pi(0.5 * pair_c + d_c), a1 = mod_2pi(0.5 * pair_c - d_c);
      const double b0 = mod_2pi(0.5 * pair_n + d_n), b1 = mod_2pi(0.5 * pair_n - d_n);
      const double th_p = mod_2pi(s0 + b0 - a0), th_m = mod_2pi(a1 + s2 - b1);
      // fine vertices of this cell and the linear index of the filled link
      size_t v0, v1;
      uint32_t l_fill;
      if (rt == 2) {
        v0 = (size_t)j * Mtf + 2 * i;
        v1 = v0 + 1;
        l_fill = 2 * (uint32_t)v1 + 1;
      } else {
        v0 = (size_t)(2 * j) * Mtf + i;
        v1 = v0 + Mtf;
        l_fill = 2 * (uint32_t)v1;
      }
      const double fill = expcos_draw(key, l_fill, beta, th_p, th_m, kVmFillin);
      if (rt == 2) {
        prime[v0] = make_double2(a0, s0);
        prime[v1] = make_double2(a1, fill);
      } else {
        prime[v0] = make_double2(s0, a0);
        prime[v1] = make_double2(fill, a1);
      }
      acc[0] += expcos_neg_log_pdf(beta, fill, th_p, th_m);
      // the same term for the current fine state
      double t_a0, t_a1, t_b0, t_b1, t_s0, t_s2, t_x;
      if (rt == 2) {
        const uint32_t i2 = 2 * i, i2p = (i2 + 2 == Mtf) ? 0 : i2 + 2;
        const double2 q0 = theta[(size_t)j * Mtf + i2], q1 = theta[(size_t)j * Mtf + i2 + 1];
        const double2 n0 = theta[(size_t)jp * Mtf + i2], n1 = theta[(size_t)jp * Mtf + i2 + 1];
        t_a0 = q0.x; t_a1 = q1.x; t_s0 = q0.y; t_x = q1.y; t_b0 = n0.x; t_b1 = n1.x;
        t_s2 = theta[(size_t)j * Mtf + i2p].y;
      } else {
        const uint32_t j2 = 2 * j, j2p = (j2 + 2 == Mxf) ? 0 : j2 + 2;
        const double2 q0 = theta[(size_t)j2 * Mtf + i], q1 = theta[(size_t)(j2 + 1) * Mtf + i];
        const double2 n0 = theta[(size_t)j2 * Mtf + ip], n1 = theta[(size_t)(j2 + 1) * Mtf + ip];
        t_a0 = q0.y; t_a1 = q1.y; t_s0 = q0.x; t_x = q1.x; t_b0 = n0.y; t_b1 = n1.y;
        t_s2 = theta[(size_t)j2p * Mtf + i].x;
      }
      acc[1] += expcos_neg_log_pdf(beta, mod_2pi(t_x), mod_2pi(-t_a0 + t_s0 + t_b0), mod_2pi(t_a1 + t_s2 - t_b1));
    }
  }
  block_sum<2>(acc, red);
  if (threadIdx.x == 0) {
    partial[((size_t)b * gridDim.x + blockIdx.x) * 2 + 0] = acc[0];
    partial[((size_t)b * gridDim.x + blockIdx.x) * 2 + 1] = acc[1];
  }
}

// ---- coarsening in both directions: QuenchedSchwingerConditionedFineAction (quenchedschwingerconditionedfineaction.cc:7-78,
// 207-289).  Three kernels: (A) per coarse cell, steps 1 and 2 -- uniform shifts of the two split coarse links, then the
// two interior spatial links from the Bessel-product law of their sum (the staples of the 2 x 2 block need the split
// links of the cells (i+1, j) and (i, j+1), recomputed from those cells' Philox streams); (B) per fine link
// (i, 2 jc + 1, 0), step 3 -- the ExpCos heat-bath conditional, reading what (A) wrote; (C) the conditioned fine action
// of a state.
__device__ __forceinline__ void split_pair(const RngKey &key, uint32_t cell, double2 coarse_link, double (&t)[2], double (&x)[2]) {
  double u, v;
  rng_uniforms(key, cell, P_FILLIN, 0, u, v);
  const double dt = (2. * u - 1.) * kPi, dx = (2. * v - 1.) * kPi;
  t[0] = mod_2pi(0.5 * coarse_link.x + dt);
  t[1] = mod_2pi(0.5 * coarse_link.x - dt);
  x[0] = mod_2pi(0.5 * coarse_link.y + dx);
  x[1] = mod_2pi(0.5 * coarse_link.y - dx);
}

__global__ void __launch_bounds__(256)
    schwinger_both_fill_kernel(uint32_t Mtc, uint32_t Mxc, BesselFill P, const double2 *__restrict__ coarse_all,
                               double2 *__restrict__ prime_all, RngKey key0) {
  const uint32_t b = blockIdx.y, Mtf = 2 * Mtc;
  const double2 *coarse = coarse_all + (size_t)b * Mtc * Mxc;
  double *prime = (double *)(prime_all + (size_t)b * 4 * Mtc * Mxc);
  RngKey key = key0;
  key.chain += b;
  for (uint32_t j = blockIdx.x; j < Mxc; j += gridDim.x) {
    const uint32_t jp = j + 1 == Mxc ? 0 : j + 1;
    for (uint32_t i = threadIdx.x; i < Mtc; i += blockDim.x) {
      const uint32_t ip = i + 1 == Mtc ? 0 : i + 1;
      const uint32_t c = j * Mtc + i, c_t = j * Mtc + ip, c_x = jp * Mtc + i;
      double t[2], x[2], tt[2], tx[2], xt[2], xx[2];
      split_pair(key, c, coarse[c], t, x);         // this cell
      split_pair(key, c_t, coarse[c_t], tt, tx);   // cell (i+1, j): its spatial pair closes the block on the right
      split_pair(key, c_x, coarse[c_x], xt, xx);   // cell (i, j+1): its temporal pair closes the block on top
      // theta_p = th(2i+1,2j,0) + th(2i+2,2j,1) + th(2i+2,2j+1,1) - th(2i+1,2j+2,0)
      const double theta_p = mod_2pi(t[1] + tx[0] + tx[1] - xt[1]);
      // theta_m = th(2i,2j,1) + th(2i,2j+1,1) + th(2i,2j+2,0) - th(2i,2j,0)
      const double theta_m = mod_2pi(x[0] + x[1] + xt[0] - t[0]);
      const double tilde = P.approximate ? approx_bessel_draw(key, c, P.beta, theta_p, theta_m)
                                         : bessel_product_draw(key, c, P, theta_p, theta_m);
      double u, v;
      rng_uniforms(key, c, P_FILLIN, 1, u, v);
      const double d = (2. * u - 1.) * kPi;
      // fine vertices (2i, 2j), (2i+1, 2j), (2i, 2j+1), (2i+1, 2j+1); link index = 2 * vertex + mu
      const size_t v00 = (size_t)(2 * j) * Mtf + 2 * i, v01 = v00 + Mtf;
      prime[2 * v00] = t[0];
      prime[2 * v00 + 1] = x[0];
      prime[2 * (v00 + 1)] = t[1];
      prime[2 * (v00 + 1) + 1] = mod_2pi(0.5 * tilde + d);
      prime[2 * v01 + 1] = x[1];
      prime[2 * (v01 + 1) + 1] = mod_2pi(0.5 * tilde - d);
    }
  }
}

// step 3: links (i, 2 jc + 1, 0), i = 0..Mt-1, jc = 0..Mx/2-1
__global__ void __launch_bounds__(256)
    schwinger_both_rows_kernel(uint32_t Mt, uint32_t Mx, double beta, double2 *__restrict__ prime_all, RngKey key0) {
  const uint32_t b = blockIdx.y;
  double *prime = (double *)(prime_all + (size_t)b * Mt * Mx);
  RngKey key = key0;
  key.chain += b;
  for (uint32_t jc = blockIdx.x; jc < Mx / 2; jc += gridDim.x) {
    const uint32_t j0 = 2 * jc, j1 = j0 + 1, j2 = (j0 + 2 == Mx) ? 0 : j0 + 2;
    for (uint32_t i = threadIdx.x; i < Mt; i += blockDim.x) {
      const uint32_t ip = i + 1 == Mt ? 0 : i + 1;
      auto link = [&](uint32_t ii, uint32_t jj, uint32_t mu) { return prime[2 * ((size_t)jj * Mt + ii) + mu]; };
      const double theta_p = mod_2pi(link(i, j0, 0) + link(ip, j0, 1) - link(i, j0, 1));
      const double theta_m = mod_2pi(link(i, j1, 1) + link(i, j2, 0) - link(ip, j1, 1));
      const uint32_t l = 2 * (j1 * Mt + i);
      prime[l] = expcos_draw(key, l, beta, theta_p, theta_m, kVmFillin);
    }
  }
}

// partial[(b * gridDim.x + blockIdx.x) * 2 + slot] = conditioned fine action of `state`, one 2 x 2 block per thread
__global__ void __launch_bounds__(256)
    schwinger_both_cfa_kernel(uint32_t Mt, uint32_t Mx, BesselFill P, const double2 *__restrict__ state_all,
                              double *__restrict__ partial, uint32_t slot) {
  __shared__ double red[4];
  const uint32_t b = blockIdx.y;
  const double *th = (const double *)(state_all + (size_t)b * Mt * Mx);
  auto link = [&](uint32_t ii, uint32_t jj, uint32_t mu) { return th[2 * ((size_t)jj * Mt + ii) + mu]; };
  double acc[1] = {0.0};
  for (uint32_t jc = blockIdx.x; jc < Mx / 2; jc += gridDim.x) {
    const uint32_t j0 = 2 * jc, j1 = j0 + 1, j2 = (j0 + 2 == Mx) ? 0 : j0 + 2;
    for (uint32_t ic = threadIdx.x; ic < Mt / 2; ic += blockDim.x) {
      const uint32_t i0 = 2 * ic, i1 = i0 + 1, i2 = (i0 + 2 == Mt) ? 0 : i0 + 2;
      if (!P.approximate) {
        const double phi_12 = +link(i0, j1, 1) + link(i0, j2, 0);
        const double phi_23 = +link(i1, j2, 0) - link(i2, j1, 1);
        const double phi_34 = -link(i1, j0, 0) - link(i2, j0, 1);
        const double phi_41 = -link(i0, j0, 0) + link(i0, j0, 1);
        const double theta_1 = +link(i0, j1, 0), theta_2 = -link(i1, j1, 1), theta_3 = -link(i1, j1, 0),
                     theta_4 = +link(i1, j0, 1);
        const double Phi = phi_12 + phi_23 + phi_34 + phi_41;
        acc[0] -= P.beta * (cos(theta_1 - theta_2 - phi_12) + cos(theta_2 - theta_3 - phi_23) +
                            cos(theta_3 - theta_4 - phi_34) + cos(theta_4 - theta_1 - phi_41));
        acc[0] -= log(bessel_znorm_inv_rescaled(P, Phi));
      } else {
        const double phi_p = mod_2pi(+link(i1, j0, 0) + link(i2, j0, 1) + link(i2, j1, 1) - link(i1, j2, 0));
        const double phi_m = mod_2pi(-link(i0, j0, 0) + link(i0, j0, 1) + link(i0, j1, 1) + link(i0, j2, 0));
        const double theta = mod_2pi(+link(i1, j0, 1) + link(i1, j1, 1));
        acc[0] -= log(approx_bessel_pdf(P.beta, theta, phi_p, phi_m));
        // the two horizontal links (i0, j1, 0), (i1, j1, 0) of this block
        for (uint32_t r = 0; r < 2; ++r) {
          const uint32_t i = i0 + r, ip = (r == 0) ? i1 : i2;
          const double hp = mod_2pi(-link(i, j0, 1) + link(i, j0, 0) + link(ip, j0, 1));
          const double hm = mod_2pi(+link(i, j1, 1) + link(i, j2, 0) - link(ip, j1, 1));
          acc[0] += expcos_neg_log_pdf(P.beta, mod_2pi(link(i, j1, 0)), hp, hm);
        }
      }
    }
  }
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) partial[((size_t)b * gridDim.x + blockIdx.x) * 2 + slot] = acc[0];
}

// QuenchedSchwingerGaussianConditionedFineAction (quenchedschwingerconditionedfineaction.cc:81-134, 293-327): the Gaussian
// variant of the fill-in for lattices coarsened in both directions.  One thread per coarse cell = one 2 x 2 block of fine
// vertices: the perimeter links come from the uniform splits of the coarse links (this cell's and, for the far sides, the
// cells (i+1, j) and (i, j+1), recomputed from their Philox streams as in schwinger_both_fill_kernel); the four interior
// links from GaussianFillinDistribution::draw.
__global__ void __launch_bounds__(256)
    schwinger_gauss_fill_kernel(uint32_t Mtc, uint32_t Mxc, double beta, const double2 *__restrict__ coarse_all,
                                double2 *__restrict__ prime_all, RngKey key0) {
  const uint32_t b = blockIdx.y, Mtf = 2 * Mtc;
  const double2 *coarse = coarse_all + (size_t)b * Mtc * Mxc;
  double2 *prime = prime_all + (size_t)b * 4 * Mtc * Mxc;
  RngKey key = key0;
  key.chain += b;
  for (uint32_t j = blockIdx.x; j < Mxc; j += gridDim.x) {
    const uint32_t jp = j + 1 == Mxc ? 0 : j + 1;
    for (uint32_t i = threadIdx.x; i < Mtc; i += blockDim.x) {
      const uint32_t ip = i + 1 == Mtc ? 0 : i + 1;
      const uint32_t c = j * Mtc + i, c_t = j * Mtc + ip, c_x = jp * Mtc + i;
      double t[2], x[2], tt[2], tx[2], xt[2], xx[2];
      split_pair(key, c, coarse[c], t, x);
      split_pair(key, c_t, coarse[c_t], tt, tx);
      split_pair(key, c_x, coarse[c_x], xt, xx);
      const double phi_12 = mod_2pi(+x[1] + xt[0]);    // th(2i, 2j+1, 1) + th(2i, 2j+2, 0)
      const double phi_23 = mod_2pi(+xt[1] - tx[1]);   // th(2i+1, 2j+2, 0) - th(2i+2, 2j+1, 1)
      const double phi_34 = mod_2pi(-tx[0] - t[1]);    // -th(2i+2, 2j, 1) - th(2i+1, 2j, 0)
      const double phi_41 = mod_2pi(-t[0] + x[0]);     // -th(2i, 2j, 0) + th(2i, 2j, 1)
      double th[4];
      gaussfill_draw(key, c, beta, phi_12, phi_23, phi_34, phi_41, th);
      const size_t v00 = (size_t)(2 * j) * Mtf + 2 * i, v01 = v00 + Mtf;
      prime[v00] = make_double2(t[0], x[0]);
      prime[v00 + 1] = make_double2(t[1], +th[3]);     // (2i+1, 2j): temporal half, interior spatial link theta_4
      prime[v01] = make_double2(+th[0], x[1]);         // (2i, 2j+1): interior temporal link theta_1, spatial half
      prime[v01 + 1] = make_double2(-th[2], -th[1]);   // (2i+1, 2j+1): -theta_3, -theta_2
    }
  }
}

// partial[(b * gridDim.x + blockIdx.x) * 2 + slot] = -sum log pdf over the 2 x 2 blocks of `state`
__global__ void __launch_bounds__(256)
    schwinger_gauss_cfa_kernel(uint32_t Mt, uint32_t Mx, double beta, const double2 *__restrict__ state_all, double *__restrict__ partial,
                               uint32_t slot) {
  __shared__ double red[4];
  const uint32_t b = blockIdx.y;
  const double *th = (const double *)(state_all + (size_t)b * Mt * Mx);
  auto link = [&](uint32_t ii, uint32_t jj, uint32_t mu) { return th[2 * ((size_t)jj * Mt + ii) + mu]; };
  double acc[1] = {0.0};
  for (uint32_t jc = blockIdx.x; jc < Mx / 2; jc += gridDim.x) {
    const uint32_t j0 = 2 * jc, j1 = j0 + 1, j2 = (j0 + 2 == Mx) ? 0 : j0 + 2;
    for (uint32_t ic = threadIdx.x; ic < Mt / 2; ic += blockDim.x) {
      const uint32_t i0 = 2 * ic, i1 = i0 + 1, i2 = (i0 + 2 == Mt) ? 0 : i0 + 2;
      const double phi_12 = mod_2pi(+link(i0, j1, 1) + link(i0, j2, 0));
      const double phi_23 = mod_2pi(+link(i1, j2, 0) - link(i2, j1, 1));
      const double phi_34 = mod_2pi(-link(i2, j0, 1) - link(i1, j0, 0));
      const double phi_41 = mod_2pi(-link(i0, j0, 0) + link(i0, j0, 1));
      const double theta_1 = mod_2pi(+link(i0, j1, 0)), theta_2 = mod_2pi(-link(i1, j1, 1)), theta_3 = mod_2pi(-link(i1, j1, 0)),
                   theta_4 = mod_2pi(+link(i1, j0, 1));
      acc[0] -= log(gaussfill_pdf(beta, theta_1, theta_2, theta_3, theta_4, phi_12, phi_23, phi_34, phi_41));
    }
  }
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) partial[((size_t)b * gridDim.x + blockIdx.x) * 2 + slot] = acc[0];
}

// en4 = [4][B]: S_f(theta'), S_f(theta), S_c(theta_C), S_c(phi_c); twolevelmetropolisstep.cc:46-84
__global__ void __launch_bounds__(256)
    lattice_twolevel_accept_kernel(uint32_t n, double *__restrict__ theta, const double *__restrict__ theta_prime,
                                   const double *__restrict__ en4, const double *__restrict__ cfa_partial, uint32_t nblk,
                                   uint32_t B, int32_t *__restrict__ accept, double *__restrict__ terms, RngKey key0) {
  const uint32_t b = blockIdx.y;
  double cfa_p = 0.0, cfa_c = 0.0;
  for (uint32_t k = 0; k < nblk; ++k) {
    cfa_p += cfa_partial[((size_t)b * nblk + k) * 2 + 0];
    cfa_c += cfa_partial[((size_t)b * nblk + k) * 2 + 1];
  }
  const double dS_fine = en4[b] - en4[B + b];
  const double dS_coarse = en4[2 * B + b] - en4[3 * B + b];
  const double dS_trial = cfa_c - cfa_p;
  const double dS = dS_fine + dS_coarse + dS_trial;
  bool acc;
  if (dS < 0.0) {
    acc = true;
  } else {
    RngKey key = key0;
    key.chain += b;
    double u, v;
    rng_uniforms(key, 0, P_ACCEPT2, 0, u, v);
    acc = u < exp(-dS);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    accept[b] = acc ? 1 : 0;
    if (terms) {
      terms[3 * b + 0] = dS_fine; terms[3 * b + 1] = dS_coarse; terms[3 * b + 2] = dS_trial;
    }
  }
  if (!acc) return;
  const size_t off = (size_t)b * n;
  for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < n; l += gridDim.x * blockDim.x)
    theta[off + l] = theta_prime[off + l];
}

}  // namespace mlmcpi

extern "C" {

// besselproductdistribution.hh:44-72: I0(2 beta), the envelope width and the Fourier coefficients alpha_k of the
// normalisation constant (k <= 16, sums truncated at n, m <= 32)
static BesselFill make_bessel_fill(double beta) {
  static BesselFill cached;
  static bool have = false;
  static std::mutex guard;
  std::lock_guard<std::mutex> lock(guard);
  if (have && cached.beta == beta) return cached;
  BesselFill P;
  P.beta = beta;
  P.approximate = beta > 8.0 ? 1 : 0;
  P.I0_twobeta = std::cyl_bessel_i(0.0, 2. * beta);
  P.sigma_beta = kPi / std::sqrt(2. * std::log(P.I0_twobeta));
  double logfact[65];
  logfact[0] = logfact[1] = 0.0;
  for (int n = 2; n <= 64; ++n) logfact[n] = logfact[n - 1] + std::log((double)n);
  auto log_binom = [&](int n, int k) { return logfact[n] - logfact[k] - logfact[n - k]; };
  double alpha0 = 1.0;
  for (int k = 0; k <= 16; ++k) {
    double sum = 0.0;
    for (int n = k; n <= 32; ++n)
      for (int m = k; m <= 32; ++m)
        sum += std::pow(0.5 * beta, 2.0 * (n + m)) *
               std::exp(log_binom(2 * n, n - k) + log_binom(2 * m, m - k) - 2 * (logfact[n] + logfact[m]));
    const double alpha = ((k == 0) ? 2 : 4) * kPi * sum;
    if (k == 0) alpha0 = alpha;
    P.alphaZ[k] = (k == 0) ? alpha : alpha / alpha0;
  }
  cached = P;
  have = true;
  return P;
}

static int check_twolevel(const mlmcpi_lattice_action *fine, const mlmcpi_lattice_action *coarse, uint32_t *rt, uint32_t *rx) {
  if (int rc = check_lattice(fine)) return rc;
  if (int rc = check_lattice(coarse)) return rc;
  if (int rc = refuse_sigma(fine, "the two-level step")) return rc;
  if (int rc = refuse_sigma(coarse, "the two-level step")) return rc;
  if (fine->kind != MLMCPI_SCHWINGER || coarse->kind != MLMCPI_SCHWINGER)
    return fail(MLMCPI_ERR_UNSUPPORTED, "two-level step: only the quenched Schwinger action has a device conditioned fine action");
  *rt = (coarse->Mt && fine->Mt == 2 * coarse->Mt) ? 2 : (fine->Mt == coarse->Mt ? 1 : 0);
  *rx = (coarse->Mx && fine->Mx == 2 * coarse->Mx) ? 2 : (fine->Mx == coarse->Mx ? 1 : 0);
  if (*rt == 0 || *rx == 0 || *rt * *rx == 1)
    return fail(MLMCPI_ERR_INVALID, "invalid coarsening for fill-in (%u x %u from %u x %u)", coarse->Mt, coarse->Mx, fine->Mt, fine->Mx);
  return MLMCPI_OK;
}

// workspace: theta' | theta_C | energies [4][B] | CFA partials [B * nblk * 2]
int mlmcpi_lattice_twolevel_workspace_bytes(const mlmcpi_lattice_action *fine, const mlmcpi_lattice_action *coarse,
                                            uint32_t B, size_t *bytes) {
  uint32_t rt, rx;
  if (int rc = check_twolevel(fine, coarse, &rt, &rx)) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  const size_t nf = (size_t)2 * fine->Mt * fine->Mx, nc = (size_t)2 * coarse->Mt * coarse->Mx;
  *bytes = align256((size_t)B * nf * 8) + align256((size_t)B * nc * 8) + align256((size_t)4 * B * 8) +
           align256((size_t)B * row_blocks(coarse->Mx, B) * 2 * 8);
  return MLMCPI_OK;
}

int mlmcpi_lattice_twolevel_draw(const mlmcpi_lattice_action *fine, const mlmcpi_lattice_action *coarse,
                                 const double *d_phi_coarse, double *d_theta, uint32_t B, uint64_t seed, uint32_t chain0,
                                 uint32_t step, void *d_work, int32_t *d_accept, double *d_terms, void *stream) {
  return mlmcpi_lattice_twolevel_draw_cfa(fine, coarse, 0, d_phi_coarse, d_theta, B, seed, chain0, step, d_work, d_accept, d_terms,
                                          stream);
}

int mlmcpi_lattice_twolevel_draw_cfa(const mlmcpi_lattice_action *fine, const mlmcpi_lattice_action *coarse, int32_t cfa_kind,
                                     const double *d_phi_coarse, double *d_theta, uint32_t B, uint64_t seed, uint32_t chain0,
                                     uint32_t step, void *d_work, int32_t *d_accept, double *d_terms, void *stream) {
  uint32_t rt, rx;
  if (int rc = check_twolevel(fine, coarse, &rt, &rx)) return rc;
  MLMCPI_REQUIRE(d_phi_coarse && d_theta && d_work && d_accept && B > 0, "bad arguments");
  MLMCPI_REQUIRE(cfa_kind == 0 || cfa_kind == 1, "unknown conditioned fine action %d", cfa_kind);
  MLMCPI_REQUIRE(cfa_kind == 0 || rt * rx == 4, "the Gaussian conditioned fine action needs a lattice coarsened in both directions");
  hipStream_t st = as_stream(stream);
  const size_t nf = (size_t)2 * fine->Mt * fine->Mx, nc = (size_t)2 * coarse->Mt * coarse->Mx;
  char *w = (char *)d_work;
  double *theta_prime = (double *)w;
  w += align256((size_t)B * nf * 8);
  double *theta_c = (double *)w;
  w += align256((size_t)B * nc * 8);
  double *en4 = (double *)w;
  w += align256((size_t)4 * B * 8);
  double *cfa = (double *)w;
  const RngKey key = make_key(seed, chain0, step);
  const uint32_t nblk = row_blocks(coarse->Mx, B);
  if (rt * rx == 4 && cfa_kind == 1) {  // QuenchedSchwingerGaussianConditionedFineAction
    const dim3 grid(nblk, B), block(256);
    hipLaunchKernelGGL(schwinger_gauss_fill_kernel, grid, block, 0, st, coarse->Mt, coarse->Mx, fine->beta, (const double2 *)d_phi_coarse,
                       (double2 *)theta_prime, key);
    MLMCPI_LAUNCH_CHECK("schwinger_gauss_fill_kernel");
    hipLaunchKernelGGL(schwinger_gauss_cfa_kernel, grid, block, 0, st, fine->Mt, fine->Mx, fine->beta, (const double2 *)theta_prime, cfa, 0u);
    hipLaunchKernelGGL(schwinger_gauss_cfa_kernel, grid, block, 0, st, fine->Mt, fine->Mx, fine->beta, (const double2 *)d_theta, cfa, 1u);
    MLMCPI_LAUNCH_CHECK("schwinger_gauss_cfa_kernel");
  } else if (rt * rx == 4) {
    const BesselFill P = make_bessel_fill(fine->beta);
    const dim3 grid(nblk, B), block(256);
    hipLaunchKernelGGL(schwinger_both_fill_kernel, grid, block, 0, st, coarse->Mt, coarse->Mx, P, (const double2 *)d_phi_coarse,
                       (double2 *)theta_prime, key);
    MLMCPI_LAUNCH_CHECK("schwinger_both_fill_kernel");
    hipLaunchKernelGGL(schwinger_both_rows_kernel, grid, block, 0, st, fine->Mt, fine->Mx, fine->beta, (double2 *)theta_prime, key);
    MLMCPI_LAUNCH_CHECK("schwinger_both_rows_kernel");
    hipLaunchKernelGGL(schwinger_both_cfa_kernel, grid, block, 0, st, fine->Mt, fine->Mx, P, (const double2 *)theta_prime, cfa, 0u);
    hipLaunchKernelGGL(schwinger_both_cfa_kernel, grid, block, 0, st, fine->Mt, fine->Mx, P, (const double2 *)d_theta, cfa, 1u);
    MLMCPI_LAUNCH_CHECK("schwinger_both_cfa_kernel");
  } else {
    hipLaunchKernelGGL(schwinger_twolevel_propose_kernel, dim3(nblk, B), dim3(256), 0, st, coarse->Mt, coarse->Mx, rt,
                       fine->beta, (const double2 *)d_phi_coarse, (const double2 *)d_theta, (double2 *)theta_prime, cfa, key);
    MLMCPI_LAUNCH_CHECK("schwinger_twolevel_propose_kernel");
  }
  if (int rc = lattice_energy(fine, theta_prime, B, en4, st)) return rc;
  if (int rc = lattice_energy(fine, d_theta, B, en4 + B, st)) return rc;
  if (int rc = mlmcpi_lattice_copy_from_fine(fine, rt, rx, d_theta, theta_c, B, stream)) return rc;
  if (int rc = lattice_energy(coarse, theta_c, B, en4 + 2 * (size_t)B, st)) return rc;
  if (int rc = lattice_energy(coarse, d_phi_coarse, B, en4 + 3 * (size_t)B, st)) return rc;
  hipLaunchKernelGGL(lattice_twolevel_accept_kernel, dim3(stream_blocks(nf), B), dim3(256), 0, st, (uint32_t)nf, d_theta,
                     (const double *)theta_prime, (const double *)en4, (const double *)cfa, nblk, B, d_accept, d_terms, key);
  MLMCPI_LAUNCH_CHECK("lattice_twolevel_accept_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
