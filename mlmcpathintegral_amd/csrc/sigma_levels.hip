// sigma_levels.hip -- the O(3) nonlinear sigma model on the levels of its CoarsenRotate hierarchy (include/mlmcpi_hip.h:
// mlmcpi_sigma_level_*).  An unrotated level is the lattice of sigma2d.hip and delegates to mlmcpi_lattice_*;
// this file adds the ROTATED level (geometry: sigma_level_device.hpp) and the transfers between a level and its coarse partner.
//
// The rotated sweep keeps the canonical form of sigma2d.hip: neighbours are read as sigma(stored angles), what stays in LDS
// after an update is sigma(angles_of(sigma')), and the file is compiled without fp contraction; so a draw gives the same bits
// whatever tile, workgroup size, fuse depth or batch split the launch uses.
#include "internal.hpp"

#include "sigma_level_device.hpp"  // fp contraction is off from here on

namespace mlmcpi {

// ---- the rotated sweep kernel ----------------------------------------------------------------------------------------
// One workgroup = one TW x TH tile of plane cells (a, b) of one chain -- the E and the O vertex of every cell --, loaded with
// a halo of K cells into LDS as 2 x 3 SoA planes of canonical unit vectors; K sweeps (k < k_heat overrelaxation, the rest heat
// bath), phase E then phase O each, one barrier per phase.  E(a, b) reads O at (a, b), (a, b-1), (a-1, b), (a-1, b-1) and O(a, b)
// reads E at (a+1, b+1), (a+1, b), (a, b+1), (a, b), so sweep k updates exactly the cells whose inputs are still exact: E on
// local [k+1, W-1-k] x [k+1, HH-1-k], O on [k+1, W-2-k] x [k+1, HH-2-k]; after K sweeps that is the tile [K, K+TW) x [K, K+TH).
// The region wraps round the planes as often as needed (any plane extents >= 1; what lies beyond the tile are periodic images,
// updated like the halo and not written); tiles on the upper / right edge of planes they do not divide reach beyond them.
template <int NT>
__global__ void __launch_bounds__(NT)
    sigma_rot_sweep_kernel(SigmaLevel L, const double2 *__restrict__ src, double2 *__restrict__ dst, uint32_t TW, uint32_t TH,
                           uint32_t tiles_a, uint32_t K, uint32_t k_heat, RngKey key) {
  extern __shared__ double lds[];
  const uint32_t W = TW + 2 * K, HH = TH + 2 * K, P = W * HH;
  double *ex = lds, *ey = lds + P, *ez = lds + 2 * P, *ox = lds + 3 * P, *oy = lds + 4 * P, *oz = lds + 5 * P;
  const uint32_t b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const uint32_t a0 = (tile % tiles_a) * TW, b0 = (tile / tiles_a) * TH;
  // plane cell of local (la, lb) = ((sa + la) mod ht, (sb + lb) mod hx); sa = a0 - K mod ht, kept non-negative
  const uint32_t sa = a0 + (K / L.ht + 1) * L.ht - K, sb = b0 + (K / L.hx + 1) * L.hx - K;
  const size_t N = L.nvert();
  const double2 *s = src + b * N;
  double2 *d = dst + b * N;
  key.chain += b;

  for (uint32_t c = tid; c < P; c += NT) {
    const uint32_t la = c % W, lb = c / W;
    const uint32_t l = ((sb + lb) % L.hx) * L.ht + (sa + la) % L.ht;
    const V3 e = sigma_of(s[l]), o = sigma_of(s[L.q + l]);
    ex[c] = e.x;
    ey[c] = e.y;
    ez[c] = e.z;
    ox[c] = o.x;
    oy[c] = o.y;
    oz[c] = o.z;
  }
  __syncthreads();

  for (uint32_t k = 0; k < K; ++k) {
    const bool heat = k >= k_heat, last = k + 1 == K;
    RngKey kk = key;
    kk.step += k;
    for (uint32_t p = 0; p < 2; ++p) {
      // phase E: la in [k+1, W-1-k]; phase O: la in [k+1, W-2-k] (and the same in lb)
      const uint32_t lo = k + 1, rw = W - 2 * k - 1 - p, rh = HH - 2 * k - 1 - p;
      double *mx = p ? ox : ex, *my = p ? oy : ey, *mz = p ? oz : ez;        // the plane this phase updates
      const double *nx = p ? ex : ox, *ny = p ? ey : oy, *nz = p ? ez : oz;  // the plane it reads
      for (uint32_t t = tid; t < rw * rh; t += NT) {
        const uint32_t la = lo + t % rw, lb = lo + t / rw;
        const uint32_t c = lb * W + la;
        // the reference's order (+1,+1), (+1,-1), (-1,+1), (-1,-1)
        const uint32_t c0 = p ? c + W + 1 : c, c1 = p ? c + 1 : c - W, c2 = p ? c + W : c - 1, c3 = p ? c : c - W - 1;
        const V3 Dl = add4(V3{nx[c0], ny[c0], nz[c0]}, V3{nx[c1], ny[c1], nz[c1]}, V3{nx[c2], ny[c2], nz[c2]},
                           V3{nx[c3], ny[c3], nz[c3]});
        const uint32_t l = p * L.q + ((sb + lb) % L.hx) * L.ht + (sa + la) % L.ht;
        const double2 ang = angles_of(sigma_update(V3{mx[c], my[c], mz[c]}, Dl, heat, L.beta, kk, l));
        const V3 cv = sigma_of(ang);
        mx[c] = cv.x;
        my[c] = cv.y;
        mz[c] = cv.z;
        if (last && la >= K && la < K + TW && lb >= K && lb < K + TH && a0 + (la - K) < L.ht && b0 + (lb - K) < L.hx) {
          __builtin_nontemporal_store(ang.x, &d[l].x);
          __builtin_nontemporal_store(ang.y, &d[l].y);
        }
      }
      __syncthreads();
    }
  }
}

// ---- streaming kernels of the rotated level ------------------------------------------------------------------------------
// group partials (sigma_level_device.hpp) over the vertices of chain b: OP 0 = sigma_E . Delta_E over the E plane (the bond
// sum), OP 1 = sigma_n over all vertices (three components); workgroup (g, b) sums group g
template <int OP>
__global__ void __launch_bounds__(kGroup) sigma_rot_reduce_kernel(SigmaLevel L, const double2 *__restrict__ phi, double *__restrict__ partial) {
  constexpr int NV = OP == 0 ? 1 : 3;
  __shared__ double red[NV * (kGroup / kWave)];
  const uint32_t b = blockIdx.y, n = OP == 0 ? L.q : L.nvert(), l = blockIdx.x * kGroup + threadIdx.x;
  const double2 *p = phi + (size_t)b * L.nvert();
  double acc[NV] = {};
  if (l < n) {
    const V3 s = sigma_of(p[l]);
    if constexpr (OP == 0) {
      const uint32_t a = l % L.ht, bb = l / L.ht, am = a == 0 ? L.ht - 1 : a - 1, bm = bb == 0 ? L.hx - 1 : bb - 1;
      const V3 Dl = add4(sigma_of(p[L.q + bb * L.ht + a]), sigma_of(p[L.q + bm * L.ht + a]), sigma_of(p[L.q + bb * L.ht + am]),
                         sigma_of(p[L.q + bm * L.ht + am]));
      acc[0] = dot3(s, Dl);
    } else {
      acc[0] = s.x;
      acc[1] = s.y;
      acc[2] = s.z;
    }
  }
  block_sum<NV>(acc, red);
  if (threadIdx.x == 0)
    for (int c = 0; c < NV; ++c) partial[((size_t)b * gridDim.x + blockIdx.x) * NV + c] = acc[c];
}

// one workgroup per chain: OP 0: out[b] = scale * sum (evaluate: scale = -beta); OP 1: out[b] = |sum|^2 * scale (chi_m)
template <int OP>
__global__ void __launch_bounds__(kGroup) sigma_rot_finish_kernel(const double *__restrict__ partial, uint32_t ngroups, double scale,
                                                                  double *__restrict__ out) {
  constexpr int NV = OP == 0 ? 1 : 3;
  __shared__ double red[NV * (kGroup / kWave)];
  double v[NV];
  chain_sum<NV>(partial + (size_t)blockIdx.x * ngroups * NV, ngroups, v, red);
  if (threadIdx.x != 0) return;
  if constexpr (OP == 0) out[blockIdx.x] = scale * v[0];
  else out[blockIdx.x] = (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) * scale;
}

// initialise_state on the level's 2 n entries: the map of sigma_init_kernel (sigma2d.hip)
__global__ void __launch_bounds__(256) sigma_level_init_kernel(uint32_t N, RngKey key0, double2 *__restrict__ x) {
  const uint32_t b = blockIdx.y;
  RngKey key = key0;
  key.chain += b;
  double2 *xb = x + (size_t)b * N;
  for (uint32_t l = blockIdx.x * 256 + threadIdx.x; l < N; l += gridDim.x * 256) {
    double u, u2, dummy;
    rng_uniforms(key, 2 * l, P_INIT, 0, u, dummy);
    rng_uniforms(key, 2 * l + 1, P_INIT, 0, u2, dummy);
    xb[l] = make_double2(acos(1.0 - 2.0 * u), -kPi + 2.0 * kPi * u2);
  }
}

// NonlinearSigmaAction::copy_from_fine / copy_from_coarse: coarse vertex number x of the fine level L, fine[l] <-> coarse[c]
__global__ void __launch_bounds__(256) sigma_level_transfer_kernel(SigmaLevel L, double2 *__restrict__ fine_all, double2 *__restrict__ coarse_all,
                                                                   int to_coarse) {
  const uint32_t b = blockIdx.y, nc = L.nfineonly();
  double2 *fine = fine_all + (size_t)b * L.nvert(), *coarse = coarse_all + (size_t)b * nc;
  for (uint32_t x = blockIdx.x * 256 + threadIdx.x; x < nc; x += gridDim.x * 256) {
    uint32_t l, c;
    coarse_site(L, x, l, c);
    if (to_coarse) coarse[c] = fine[l]; else fine[l] = coarse[c];
  }
}

int check_sigma_level(const mlmcpi_sigma_level *level) {
  MLMCPI_REQUIRE(level, "level is NULL");
  MLMCPI_REQUIRE(level->Mt >= 2 && level->Mx >= 2 && level->Mt % 2 == 0 && level->Mx % 2 == 0,
                 "a sigma-model level needs even extents >= 2 (got %u x %u)", level->Mt, level->Mx);
  MLMCPI_REQUIRE((uint64_t)level->Mt * level->Mx <= (1ull << 30), "lattice too large for 32-bit site indices");
  return MLMCPI_OK;
}

namespace {

mlmcpi_lattice_action as_lattice(const mlmcpi_sigma_level *l) { return mlmcpi_lattice_action{MLMCPI_NONLINEAR_SIGMA, l->Mt, l->Mx, l->beta, 0.0}; }

struct RotPlan {
  uint32_t tw, th, nt, fuse;
};

// tile of plane cells, workgroup size and fuse depth of the rotated sweep: the option, else 32 x 32 cells, 512 threads, two
// sweeps per launch; the tile never exceeds the planes, and the LDS image (48 B per cell of the loaded region) fits
RotPlan rot_plan(const SigmaLevel &L, const Tuning &t) {
  RotPlan p{t.sigma_level_tw ? t.sigma_level_tw : 32u, t.sigma_level_th ? t.sigma_level_th : 32u, t.sigma_level_nt ? t.sigma_level_nt : 512u,
            t.sigma_level_fuse ? t.sigma_level_fuse : 2u};
  if (p.tw > L.ht) p.tw = L.ht;
  if (p.th > L.hx) p.th = L.hx;
  return p;
}

DeviceOnce g_rot_attr_once;

int rot_init_sweep_kernels() {  // the sweep kernel may take the whole LDS (of the current device)
  return once_per_device(g_rot_attr_once, []() -> int {
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_rot_sweep_kernel<256>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_rot_sweep_kernel<512>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_rot_sweep_kernel<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    return MLMCPI_OK;
  });
}

template <int OP>
int rot_reduce(const SigmaLevel &L, const double *d_phi, uint32_t B, double scale, double *d_out, hipStream_t st) {
  constexpr int NV = OP == 0 ? 1 : 3;
  const uint32_t n = OP == 0 ? L.q : L.nvert(), ng = (n + kGroup - 1) / kGroup;
  void *part = nullptr;
  if (int rc = scratch((size_t)B * ng * NV * sizeof(double), &part, st)) return rc;
  hipLaunchKernelGGL(sigma_rot_reduce_kernel<OP>, dim3(ng, B), dim3(kGroup), 0, st, L, (const double2 *)d_phi, (double *)part);
  MLMCPI_LAUNCH_CHECK("sigma_rot_reduce_kernel");
  hipLaunchKernelGGL(sigma_rot_finish_kernel<OP>, dim3(B), dim3(kGroup), 0, st, (const double *)part, ng, scale, d_out);
  MLMCPI_LAUNCH_CHECK("sigma_rot_finish_kernel");
  return MLMCPI_OK;
}

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_sigma_level_state_size(const mlmcpi_sigma_level *level, uint32_t *n) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(n, "bad arguments");
  *n = 2 * make_level(*level).nvert();
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_initialise(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint64_t seed, uint32_t chain0,
                                  void *stream) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(d_state && B > 0 && B <= 65535, "bad arguments");
  const uint32_t N = make_level(*level).nvert();
  hipLaunchKernelGGL(sigma_level_init_kernel, dim3(stream_blocks(N), B), dim3(256), 0, as_stream(stream), N, make_key(seed, chain0, 0),
                     (double2 *)d_state);
  MLMCPI_LAUNCH_CHECK("sigma_level_init_kernel");
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_evaluate(const mlmcpi_sigma_level *level, const double *d_state, uint32_t B, double *d_S, void *stream) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(d_state && d_S && B > 0 && B <= 65535, "bad arguments");
  if (!level->rotated) {
    const mlmcpi_lattice_action act = as_lattice(level);
    return mlmcpi_lattice_evaluate(&act, d_state, B, d_S, stream);
  }
  return rot_reduce<0>(make_level(*level), d_state, B, -level->beta, d_S, as_stream(stream));
}

int mlmcpi_sigma_level_magnetic_susceptibility(const mlmcpi_sigma_level *level, const double *d_state, uint32_t B, double *d_out,
                                               void *stream) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(d_state && d_out && B > 0 && B <= 65535, "bad arguments");
  if (!level->rotated) return mlmcpi_qoi_magnetic_susceptibility(d_state, level->Mt, level->Mx, B, d_out, stream);
  const SigmaLevel L = make_level(*level);
  return rot_reduce<1>(L, d_state, B, 1.0 / (double)L.nvert(), d_out, as_stream(stream));
}

int mlmcpi_sigma_level_sweep_draw(const mlmcpi_sigma_level *level, double *d_state, double *d_scratch, uint32_t B,
                                  uint32_t n_overrelax, uint32_t n_heatbath, uint64_t seed, uint32_t chain0, uint32_t sweep0,
                                  void *stream) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(d_state && d_scratch && B > 0 && B <= 65535, "bad arguments");
  if (!level->rotated) {
    const mlmcpi_lattice_action act = as_lattice(level);
    return mlmcpi_lattice_sweep_draw(&act, d_state, d_scratch, B, n_overrelax, n_heatbath, seed, chain0, sweep0, 0, stream);
  }
  const uint64_t n_sweeps = (uint64_t)n_overrelax + n_heatbath;
  MLMCPI_REQUIRE(sweep0 + n_sweeps <= 0xFFFFFFFFull, "sweep0 + the number of sweeps must fit 32 bits");
  if (n_sweeps == 0) return MLMCPI_OK;
  if (int rc = rot_init_sweep_kernels()) return rc;
  hipStream_t st = as_stream(stream);
  const SigmaLevel L = make_level(*level);
  const RotPlan plan = rot_plan(L, tuning());
  const uint32_t tiles_a = (L.ht + plan.tw - 1) / plan.tw, tiles = tiles_a * ((L.hx + plan.th - 1) / plan.th);
  const double *src = d_state;
  double *dst = d_scratch;
  for (uint32_t done = 0; done < n_sweeps;) {
    uint32_t K = (uint32_t)n_sweeps - done < plan.fuse ? (uint32_t)n_sweeps - done : plan.fuse;
    const uint32_t k_heat = done >= n_overrelax ? 0 : (n_overrelax - done < K ? n_overrelax - done : K);
    const size_t lds = (size_t)(plan.tw + 2 * K) * (plan.th + 2 * K) * 6 * sizeof(double);
    MLMCPI_REQUIRE(lds <= kSigmaLdsMax, "the rotated sweep's tile does not fit the LDS");
    const RngKey key = make_key(seed, chain0, sweep0 + done);
#define MLMCPI_ROT_SWEEP(NT)                                                                                                       \
  hipLaunchKernelGGL(sigma_rot_sweep_kernel<NT>, dim3(tiles, B), dim3(NT), lds, st, L, (const double2 *)src, (double2 *)dst, plan.tw, \
                     plan.th, tiles_a, K, k_heat, key)
    if (plan.nt == 1024) MLMCPI_ROT_SWEEP(1024);
    else if (plan.nt == 512) MLMCPI_ROT_SWEEP(512);
    else MLMCPI_ROT_SWEEP(256);
#undef MLMCPI_ROT_SWEEP
    MLMCPI_LAUNCH_CHECK("sigma_rot_sweep_kernel");
    done += K;
    src = dst;
    dst = dst == d_scratch ? d_state : d_scratch;
  }
  if (src != d_state) MLMCPI_HIP_TRY(hipMemcpyAsync(d_state, src, (size_t)B * 2 * L.nvert() * sizeof(double), hipMemcpyDeviceToDevice, st));
  return MLMCPI_OK;
}

static int level_transfer(const mlmcpi_sigma_level *fine, double *d_fine, double *d_coarse, uint32_t B, int to_coarse, void *stream) {
  if (int rc = check_sigma_level(fine)) return rc;
  MLMCPI_REQUIRE(d_fine && d_coarse && B > 0 && B <= 65535, "bad arguments");
  const SigmaLevel L = make_level(*fine);
  hipLaunchKernelGGL(sigma_level_transfer_kernel, dim3(stream_blocks(L.nfineonly()), B), dim3(256), 0, as_stream(stream), L,
                     (double2 *)d_fine, (double2 *)d_coarse, to_coarse);
  MLMCPI_LAUNCH_CHECK("sigma_level_transfer_kernel");
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_copy_from_fine(const mlmcpi_sigma_level *fine, const double *d_fine, double *d_coarse, uint32_t B,
                                      void *stream) {
  return level_transfer(fine, (double *)d_fine, d_coarse, B, 1, stream);
}

int mlmcpi_sigma_level_copy_from_coarse(const mlmcpi_sigma_level *fine, const double *d_coarse, double *d_fine, uint32_t B,
                                        void *stream) {
  return level_transfer(fine, d_fine, (double *)d_coarse, B, 0, stream);
}

}  // extern "C"
