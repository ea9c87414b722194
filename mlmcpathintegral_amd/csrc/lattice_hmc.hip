// lattice_hmc.hip -- force of the GFF and Schwinger actions and the generic 2-D HMC built on it (the leapfrog step fuses
// the force with the momentum and position updates, so the two share the force's device code).
#include "internal.hpp"

namespace mlmcpi {

// gffaction.cc:80-94
__global__ void __launch_bounds__(256) gff_force_kernel(uint32_t Mt, uint32_t Mx, double mu2,
                                                        const double *__restrict__ phi_all, double *__restrict__ f_all) {
  const uint32_t b = blockIdx.y;
  const double *phi = phi_all + (size_t)b * Mt * Mx;
  double *f = f_all + (size_t)b * Mt * Mx;
  const double kappa = 4. + mu2;
  for (uint32_t j = blockIdx.x; j < Mx; j += gridDim.x) {
    const uint32_t jm = j == 0 ? Mx - 1 : j - 1, jp = j + 1 == Mx ? 0 : j + 1;
    for (uint32_t i = threadIdx.x; i < Mt; i += blockDim.x) {
      const uint32_t im = i == 0 ? Mt - 1 : i - 1, ip = i + 1 == Mt ? 0 : i + 1;
      double m = kappa * phi[(size_t)j * Mt + i];
      m -= phi[(size_t)j * Mt + ip];
      m -= phi[(size_t)j * Mt + im];
      m -= phi[(size_t)jp * Mt + i];
      m -= phi[(size_t)jm * Mt + i];
      f[(size_t)j * Mt + i] = m;
    }
  }
}

// Gather form of quenchedschwingeraction.cc:68-89: the reference scatters +-beta sin(theta_P) of
// plaquette (i,j) onto its four links; link (i,j,0) therefore receives F(i,j) - F(i,j-1) and link
// (i,j,1) receives F(i-1,j) - F(i,j) (each a two-term sum, so the value is order independent).
//
// One sine per plaquette.  (Until r03 every thread computed the three plaquettes its two links touch -- three sines per
// site, 0.37 ms for 1024^2 x 32 = 0.36 of the HBM roofline for a kernel that reads and writes the state once.)  A WAVE
// walks up a band of rows with 64 consecutive columns: lane l holds column (62 tile + l - 1) mod Mt, takes theta_1 of the
// column to its right from lane l + 1 and F of the column to its left from lane l - 1 (DPP rotations: no LDS, no barrier),
// and keeps F of the row below in a register.  Lanes 1 .. 62 emit; lane 0 only supplies F, lane 63 only theta_1: tiles step
// by 62 columns, 3 % redundant loads and sines, and nothing at the edge of a wave is special.  Rows are loaded two ahead
// of their use.  Same arithmetic per plaquette as before (same sum order): bit-identical forces.
#ifndef MLMCPI_FORCE_ROWS
#define MLMCPI_FORCE_ROWS 128
#endif
constexpr uint32_t kForceCols = 62, kForceRows = MLMCPI_FORCE_ROWS;
__host__ __device__ inline uint32_t force_waves(uint32_t Mt, uint32_t Mx) {
  return ((Mt + kForceCols - 1) / kForceCols) * ((Mx + kForceRows - 1) / kForceRows);
}
// emit(j, i, F_0, F_1): force on the two links of vertex (i, j)
template <class Emit>
__device__ __forceinline__ void schwinger_force_band(const double2 *__restrict__ t, uint32_t Mt, uint32_t Mx, double coupling,
                                                     uint32_t wave_id, Emit emit) {
  const uint32_t tiles = (Mt + kForceCols - 1) / kForceCols;
  const uint32_t band = wave_id / tiles, tile = wave_id - band * tiles, lane = threadIdx.x & (kWave - 1);
  const uint32_t col = tile * kForceCols + lane;                       // column + 1, not wrapped
  const uint32_t i = (uint32_t)(((uint64_t)col + Mt - 1) % Mt);
  const bool owner = lane >= 1 && lane <= kForceCols && col <= Mt;     // col - 1 < Mt: not a column of the next lap
  const uint32_t jb = band * kForceRows, je = min(jb + kForceRows, Mx);
  auto up_of = [&](uint32_t j) { return j + 1 == Mx ? 0u : j + 1; };
  auto F_of = [&](const double2 &a, const double2 &above) {
    // theta(i,j,0) + theta(i+1,j,1) - theta(i,j+1,0) - theta(i,j,1)   (quenchedschwingeraction.cc:14-17)
    return coupling * sin_reduced(a.x + wave_rotate_down(a.y) - above.x - a.y);
  };
  // Rows are loaded four ahead of their use, at the TOP of an iteration (vmcnt counts stores too and retires in order, so
  // waiting for a row implies waiting for every store issued before its load).  Measured: 0.234 ms with two rows of
  // lookahead as with four, bands of 32 rows; 0.228 ms with bands of 128 (fewer band edges); EXPERIMENTS 1.6.
  const uint32_t jm = jb == 0 ? Mx - 1 : jb - 1;
  uint32_t jn = jb;
  auto next_row = [&]() {   // (up to four rows past the band at its end: valid rows, not used -- guarding the load cost 5 %)
    jn = up_of(jn);
    return t[(size_t)jn * Mt + i];
  };
  const double2 below = t[(size_t)jm * Mt + i];
  double2 here = t[(size_t)jb * Mt + i], above = next_row(), ahead1 = next_row(), ahead2 = next_row();
  double F_below = F_of(below, here);
  for (uint32_t j = jb; j < je; ++j) {
    const double2 ahead3 = next_row();
    const double F = F_of(here, above);
    const double F_left = wave_rotate_up(F);
    if (owner) emit(j, i, F - F_below, F_left - F);
    F_below = F;
    here = above;
    above = ahead1;
    ahead1 = ahead2;
    ahead2 = ahead3;
  }
}

// grid (ceil(force_waves / 4), B)
__global__ void __launch_bounds__(256) schwinger_force_kernel(uint32_t Mt, uint32_t Mx, double beta,
                                                              const double2 *__restrict__ t_all,
                                                              double2 *__restrict__ f_all) {
  const uint32_t b = blockIdx.y, wave_id = blockIdx.x * 4 + threadIdx.x / kWave;
  if (wave_id >= force_waves(Mt, Mx)) return;   // (a whole wave)
  double2 *f = f_all + (size_t)b * Mt * Mx;
  schwinger_force_band(t_all + (size_t)b * Mt * Mx, Mt, Mx, beta, wave_id,
                       // (non-temporal stores, r05: 0.227 -> 0.221 ms over three same-box pairs, 0.59 -> 0.61 of 8 TB/s by the floor bytes)
                       [&](uint32_t j, uint32_t i, double f0, double f1) { store_streaming(&f[(size_t)j * Mt + i], f0, f1); });
}

// =================================================================================================
// Generic HMC for 2-D actions (sampler/hmcsampler.cc:8-69), streaming form: momenta and the trial
// state live in HBM, one fused force + momentum + position kernel per leapfrog step (ping-pong on
// the trial state because neighbours need the old positions).
// =================================================================================================

// p ~ N(0,1) per entry (Philox site = entry index), trial <- current
__global__ void __launch_bounds__(256)
    lat_hmc_init_kernel(uint32_t n, const double *__restrict__ x_cur, double *__restrict__ x_trial,
                        double *__restrict__ p, const int32_t *__restrict__ done, RngKey key0) {
  const uint32_t b = blockIdx.y;
  if (done[b]) return;
  RngKey key = key0;
  key.chain += b;
  const size_t off = (size_t)b * n;
  for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < n; l += gridDim.x * blockDim.x) {
    p[off + l] = rng_normal0(key, l, P_MOMENTUM, 0);
    x_trial[off + l] = x_cur[off + l];
  }
}

// one leapfrog step: F(x_in); p -= dtp F; x_out = x_in + dtx p
template <int KIND>
__global__ void __launch_bounds__(256)
    lat_hmc_step_kernel(uint32_t Mt, uint32_t Mx, double coupling, const double *__restrict__ x_in,
                        double *__restrict__ x_out, double *__restrict__ p_all, const int32_t *__restrict__ done,
                        double dtp, double dtx) {
  const uint32_t b = blockIdx.y;
  if (done[b]) return;
  if (KIND == MLMCPI_GFF) {
    const double *phi = x_in + (size_t)b * Mt * Mx;
    double *out = x_out + (size_t)b * Mt * Mx, *p = p_all + (size_t)b * Mt * Mx;
    const double kappa = 4. + coupling;
    for (uint32_t j = blockIdx.x; j < Mx; j += gridDim.x) {
      const uint32_t jm = j == 0 ? Mx - 1 : j - 1, jp = j + 1 == Mx ? 0 : j + 1;
      for (uint32_t i = threadIdx.x; i < Mt; i += blockDim.x) {
        const uint32_t im = i == 0 ? Mt - 1 : i - 1, ip = i + 1 == Mt ? 0 : i + 1;
        const size_t o = (size_t)j * Mt + i;
        double F = kappa * phi[o];
        F -= phi[(size_t)j * Mt + ip];
        F -= phi[(size_t)j * Mt + im];
        F -= phi[(size_t)jp * Mt + i];
        F -= phi[(size_t)jm * Mt + i];
        const double pn = p[o] - dtp * F;
        p[o] = pn;
        out[o] = phi[o] + dtx * pn;
      }
    }
  } else {
    // grid (ceil(force_waves / 4), B): one sine per plaquette (schwinger_force_band)
    const uint32_t wave_id = blockIdx.x * 4 + threadIdx.x / kWave;
    if (wave_id >= force_waves(Mt, Mx)) return;
    const double2 *t = (const double2 *)x_in + (size_t)b * Mt * Mx;
    double2 *out = (double2 *)x_out + (size_t)b * Mt * Mx, *p = (double2 *)p_all + (size_t)b * Mt * Mx;
    schwinger_force_band(t, Mt, Mx, coupling, wave_id, [&](uint32_t j, uint32_t i, double f0, double f1) {
      const size_t o = (size_t)j * Mt + i;
      double2 pn = p[o];
      pn.x -= dtp * f0;
      pn.y -= dtp * f1;
      p[o] = pn;
      const double2 xo = t[o];
      out[o] = make_double2(xo.x + dtx * pn.x, xo.y + dtx * pn.y);
    });
  }
}

// en4 = [4][B]: S0, T0, S1, T1 (already scaled).  hmcsampler.cc:50-67.
__global__ void __launch_bounds__(256)
    lat_hmc_accept_kernel(uint32_t n, double *__restrict__ x_cur, const double *__restrict__ x_trial,
                          const double *__restrict__ en4, uint32_t B, const int32_t *__restrict__ done_in,
                          int32_t *__restrict__ done_out, double *__restrict__ energies, RngKey key0) {
  const uint32_t b = blockIdx.y;
  if (done_in[b]) {
    if (blockIdx.x == 0 && threadIdx.x == 0) done_out[b] = 1;
    return;
  }
  const double S0 = en4[b], T0 = en4[B + b], S1 = en4[2 * B + b], T1 = en4[3 * B + b];
  const double dH = (S1 - S0) + (T1 - T0);
  bool acc;
  if (dH < 0.0) {
    acc = true;
  } else {
    RngKey key = key0;
    key.chain += b;
    double u, v;
    rng_uniforms(key, 0, P_ACCEPT, 0, u, v);
    acc = u < exp(-dH);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    done_out[b] = acc ? 1 : 0;
    if (energies) {
      energies[4 * b + 0] = S0; energies[4 * b + 1] = T0; energies[4 * b + 2] = S1; energies[4 * b + 3] = T1;
    }
  }
  if (!acc) return;
  const size_t off = (size_t)b * n;
  for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < n; l += gridDim.x * blockDim.x)
    x_cur[off + l] = x_trial[off + l];
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_lattice_force(const mlmcpi_lattice_action *act, const double *d_phi, double *d_f, uint32_t B,
                         void *stream) {
  if (int rc = check_lattice(act)) return rc;
  MLMCPI_REQUIRE(d_phi && d_f && d_phi != d_f && B > 0, "bad arguments");
  if (act->kind == MLMCPI_NONLINEAR_SIGMA) return sigma_force(act, d_phi, d_f, B, as_stream(stream));
  dim3 grid(row_blocks(act->Mx, B), B), block(256);
  if (act->kind == MLMCPI_GFF)
    hipLaunchKernelGGL(gff_force_kernel, grid, block, 0, as_stream(stream), act->Mt, act->Mx, gff_mu2(*act), d_phi, d_f);
  else
    hipLaunchKernelGGL(schwinger_force_kernel, dim3((force_waves(act->Mt, act->Mx) + 3) / 4, B), block, 0, as_stream(stream),
                       act->Mt, act->Mx, act->beta, (const double2 *)d_phi, (double2 *)d_f);
  MLMCPI_LAUNCH_CHECK("lattice force kernel");
  return MLMCPI_OK;
}

// workspace: p | trial A | trial B | energies [4][B] | flags [2][B]
int mlmcpi_lattice_hmc_workspace_bytes(const mlmcpi_lattice_action *act, uint32_t B, size_t *bytes) {
  if (int rc = check_lattice(act)) return rc;
  if (int rc = refuse_sigma(act, "HMC (in (theta, phi) the target density carries sin theta, which the reference's force leaves out)")) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  uint32_t n = 0;
  mlmcpi_lattice_state_size(act, &n);
  *bytes = 3 * align256((size_t)B * n * 8) + align256((size_t)4 * B * 8) + align256((size_t)2 * B * 4);
  return MLMCPI_OK;
}

int mlmcpi_lattice_hmc_draw(const mlmcpi_lattice_action *act, double *d_phi, uint32_t B, uint32_t nt, double dt,
                            uint32_t n_rep, uint64_t seed, uint32_t chain0, uint32_t traj0, void *d_work,
                            int32_t *d_accept, double *d_energies, void *stream) {
  if (int rc = check_lattice(act)) return rc;
  if (int rc = refuse_sigma(act, "HMC (in (theta, phi) the target density carries sin theta, which the reference's force leaves out)")) return rc;
  MLMCPI_REQUIRE(d_phi && d_work && B > 0 && n_rep > 0, "bad arguments");
  uint32_t n = 0;
  mlmcpi_lattice_state_size(act, &n);
  hipStream_t st = as_stream(stream);
  char *w = (char *)d_work;
  const size_t sb = align256((size_t)B * n * 8);
  double *p = (double *)w, *xa = (double *)(w + sb), *xb = (double *)(w + 2 * sb);
  double *en4 = (double *)(w + 3 * sb);
  int32_t *flags = (int32_t *)(w + 3 * sb + align256((size_t)4 * B * 8));
  MLMCPI_HIP_TRY(hipMemsetAsync(flags, 0, (size_t)2 * B * 4, st));
  const dim3 lin_grid(stream_blocks(n), B), row_grid(row_blocks(act->Mx, B), B), block(256);
  const double coupling = act->kind == MLMCPI_GFF ? gff_mu2(*act) : act->beta;
  for (uint32_t r = 0; r < n_rep; ++r) {
    const int32_t *done_in = flags + (size_t)(r & 1) * B;
    int32_t *done_out = flags + (size_t)((r + 1) & 1) * B;
    const RngKey key = make_key(seed, chain0, traj0 + r);
    hipLaunchKernelGGL(lat_hmc_init_kernel, lin_grid, block, 0, st, n, (const double *)d_phi, xa, p, done_in, key);
    MLMCPI_LAUNCH_CHECK("lat_hmc_init_kernel");
    if (int rc = lattice_energy(act, d_phi, B, en4, st)) return rc;
    if (int rc = lattice_sum_squares(p, n, B, 0.5, en4 + B, st)) return rc;
    double *src = xa, *dst = xb;
    for (uint32_t k = 0; k <= nt; ++k) {
      const double dtp = (k == 0 || k == nt) ? 0.5 * dt : dt;
      const double dtx = (k == nt) ? 0.0 : dt;
      if (act->kind == MLMCPI_GFF)
        hipLaunchKernelGGL(lat_hmc_step_kernel<MLMCPI_GFF>, row_grid, block, 0, st, act->Mt, act->Mx, coupling,
                           (const double *)src, dst, p, done_in, dtp, dtx);
      else
        hipLaunchKernelGGL(lat_hmc_step_kernel<MLMCPI_SCHWINGER>, dim3((force_waves(act->Mt, act->Mx) + 3) / 4, B), block, 0, st, act->Mt, act->Mx, coupling,
                           (const double *)src, dst, p, done_in, dtp, dtx);
      MLMCPI_LAUNCH_CHECK("lat_hmc_step_kernel");
      double *tmp = src; src = dst; dst = tmp;
    }
    if (int rc = lattice_energy(act, src, B, en4 + 2 * (size_t)B, st)) return rc;
    if (int rc = lattice_sum_squares(p, n, B, 0.5, en4 + 3 * (size_t)B, st)) return rc;
    hipLaunchKernelGGL(lat_hmc_accept_kernel, lin_grid, block, 0, st, n, d_phi, (const double *)src,
                       (const double *)en4, B, done_in, done_out, d_energies, key);
    MLMCPI_LAUNCH_CHECK("lat_hmc_accept_kernel");
  }
  if (d_accept)
    MLMCPI_HIP_TRY(hipMemcpyAsync(d_accept, flags + (size_t)(n_rep & 1) * B, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
  return MLMCPI_OK;
}

}  // extern "C"
