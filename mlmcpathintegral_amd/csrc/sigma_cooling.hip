// sigma_cooling.hip -- cooling of an O(3) sigma-model field on a level, rotated or not, and the charge, susceptibility and energy
// of the cooled field at a list of depths (include/mlmcpi_hip.h: mlmcpi_sigma_level_cooled_charge).
//
//   sigma_l <- Delta_l / |Delta_l|,  Delta_l = add4 of the four neighbours in the reference's order,  |Delta| = sqrt((x^2 + y^2) + z^2)
//
// the deterministic beta -> infinity limit of the heat bath; Delta_l = 0 leaves sigma_l as it is.  One sweep = the two colour
// classes in the sweeps' order (plain: (i + j) even, then odd; rotated: phase E, then phase O).  The Markov chain's state is only
// read: the field lives in the caller's workspace as unit vectors, per chain three planes x[n], y[n], z[n] in the level's vertex
// order, and is never converted back to angles.
//
// The smoother of a call of the smoothing driver (sigma_smooth.hip: the field is staged, smoothed between two buffers, measured at
// each listed depth and turned back into angles by sigma_field.hip's launches) is
//   sigma_cool_kernel<ROT, NT>: one workgroup per tile per chain loads TW x TH vertices (rotated: plane cells, E and O) plus the
//   halo K fused sweeps need (plain 2 K vertices, sigma2d.hip; rotated K cells, sigma_levels.hip) from one buffer, runs K sweeps
//   in LDS, one barrier per phase, each phase on exactly the sites whose inputs are still exact, and writes the tile to the other
//   buffer.  Tiles that do not divide the plane and halos that pass its edge wrap with modular loads.
// An update is a pure function of four stored vectors, so a halo vertex recomputed by a neighbouring tile gets the bits its owner
// computes, and a vertex written to the buffer and loaded again is the vertex that stayed in LDS: the field of depth d does not
// depend on the tile, the workgroup size, the fuse depth or the depths listed before d.  No atomics; workgroups ride one linear
// index over grid x and then y (topo_grid).
#include "sigma_smooth_host.hpp"  // the driver; includes sigma_level_device.hpp: fp contraction is off from here on

#include "sigma_field_device.hpp"  // the field's layout

namespace mlmcpi {

__device__ __forceinline__ V3 sigma_cool(const V3 &sig, const V3 &Dl) {
  const double n2 = (Dl.x * Dl.x + Dl.y * Dl.y) + Dl.z * Dl.z;
  if (!(n2 > 0.0)) return sig;
  const double nrm = sqrt(n2);
  return V3{Dl.x / nrm, Dl.y / nrm, Dl.z / nrm};
}

// ---- the cooling kernel ------------------------------------------------------------------------------------------------------
// ROT = 0: the geometry of sigma_sweep_kernel.  Halo H = 2 K vertices, loaded region W x HH = (TW + 2 H) x (TH + 2 H), three SoA
// planes; phase m = 2 k + c + 1 (sweep k, colour c) updates the sites of colour c at least m from the edge of the region, the last
// phase exactly the tile.  A row of the phase holds ceil(rw / 2) candidates, the first of the row's colour; the one past the end
// of a row of odd length is skipped, so odd tiles run.
// ROT = 1: the geometry of sigma_rot_sweep_kernel.  Halo K cells, region (TW + 2 K) x (TH + 2 K) cells, 2 x 3 SoA planes; sweep k
// updates E on local [k+1, W-1-k] x [k+1, HH-1-k] and then O on [k+1, W-2-k] x [k+1, HH-2-k].
template <int ROT, int NT>
__global__ void __launch_bounds__(NT)
    sigma_cool_kernel(SigmaLevel L, uint64_t nblocks, const double *__restrict__ src, double *__restrict__ dst, uint32_t TW, uint32_t TH,
                      uint32_t tiles_a, uint32_t tiles, uint32_t K) {
  extern __shared__ double lds[];
  const uint64_t wg = topo_block();
  if (wg >= nblocks) return;
  const uint32_t tile = (uint32_t)(wg % tiles), tid = threadIdx.x, n = L.nvert();
  const double *s = src + (wg / tiles) * 3 * n;
  double *d = dst + (wg / tiles) * 3 * n;
  const uint32_t PW = ROT ? L.ht : L.Mt, PH = ROT ? L.hx : L.Mx;  // the plane
  const uint32_t H = ROT ? K : 2 * K, W = TW + 2 * H, HH = TH + 2 * H, P = W * HH;
  const uint32_t a0 = (tile % tiles_a) * TW, b0 = (tile / tiles_a) * TH;
  // plane entry of local (la, lb) = ((sa + la) mod PW, (sb + lb) mod PH); sa = a0 - H mod PW, kept non-negative
  const uint32_t sa = a0 + (H / PW + 1) * PW - H, sb = b0 + (H / PH + 1) * PH - H;

  for (uint32_t c = tid; c < P; c += NT) {
    const uint32_t la = c % W, lb = c / W;
    const uint32_t l = ((sb + lb) % PH) * PW + (sa + la) % PW;
    const V3 e = field_fetch(s, n, l);
    lds[c] = e.x;
    lds[P + c] = e.y;
    lds[2 * P + c] = e.z;
    if constexpr (ROT) {
      const V3 o = field_fetch(s, n, L.q + l);
      lds[3 * P + c] = o.x;
      lds[4 * P + c] = o.y;
      lds[5 * P + c] = o.z;
    }
  }
  __syncthreads();

  for (uint32_t k = 0; k < K; ++k) {
    const bool last = k + 1 == K;
    for (uint32_t p = 0; p < 2; ++p) {
      if constexpr (ROT) {
        const uint32_t lo = k + 1, rw = W - 2 * k - 1 - p, rh = HH - 2 * k - 1 - p;
        double *m = lds + (p ? 3 * P : 0);          // the plane this phase updates
        const double *nb = lds + (p ? 0 : 3 * P);   // the plane it reads
        for (uint32_t t = tid; t < rw * rh; t += NT) {
          const uint32_t la = lo + t % rw, lb = lo + t / rw, c = lb * W + la;
          // the reference's order (+1,+1), (+1,-1), (-1,+1), (-1,-1)
          const uint32_t c0 = p ? c + W + 1 : c, c1 = p ? c + 1 : c - W, c2 = p ? c + W : c - 1, c3 = p ? c : c - W - 1;
          const V3 Dl = add4(V3{nb[c0], nb[P + c0], nb[2 * P + c0]}, V3{nb[c1], nb[P + c1], nb[2 * P + c1]},
                             V3{nb[c2], nb[P + c2], nb[2 * P + c2]}, V3{nb[c3], nb[P + c3], nb[2 * P + c3]});
          const V3 v = sigma_cool(V3{m[c], m[P + c], m[2 * P + c]}, Dl);
          m[c] = v.x;
          m[P + c] = v.y;
          m[2 * P + c] = v.z;
          if (last && la >= K && la < K + TW && lb >= K && lb < K + TH && a0 + (la - K) < L.ht && b0 + (lb - K) < L.hx)
            field_store(d, n, p * L.q + ((sb + lb) % L.hx) * L.ht + (sa + la) % L.ht, v);
        }
      } else {
        const uint32_t m = 2 * k + p + 1, rw = W - 2 * m, rw2 = (rw + 1) / 2, rh = HH - 2 * m;
        for (uint32_t t = tid; t < rw2 * rh; t += NT) {
          const uint32_t lb = m + t / rw2;
          const uint32_t la = m + 2 * (t % rw2) + ((p + sa + sb + lb + m) & 1u);
          if (la >= W - m) continue;
          const uint32_t c = lb * W + la;
          // the reference's order (+1, 0), (-1, 0), (0, +1), (0, -1)
          const V3 Dl = add4(V3{lds[c + 1], lds[P + c + 1], lds[2 * P + c + 1]}, V3{lds[c - 1], lds[P + c - 1], lds[2 * P + c - 1]},
                             V3{lds[c + W], lds[P + c + W], lds[2 * P + c + W]}, V3{lds[c - W], lds[P + c - W], lds[2 * P + c - W]});
          const V3 v = sigma_cool(V3{lds[c], lds[P + c], lds[2 * P + c]}, Dl);
          lds[c] = v.x;
          lds[P + c] = v.y;
          lds[2 * P + c] = v.z;
          if (last && la >= H && la < H + TW && lb >= H && lb < H + TH && a0 + (la - H) < L.Mt && b0 + (lb - H) < L.Mx)
            field_store(d, n, (size_t)((sb + lb) % L.Mx) * L.Mt + (sa + la) % L.Mt, v);
        }
      }
      __syncthreads();
    }
  }
}

namespace {

// the default 32 x 32 x 512 x 2 takes 38 KB of LDS on a plain level, 62 KB on a rotated one
size_t cool_lds(const SigmaLevel &L, const SmoothPlan &p, uint32_t K) {
  const uint32_t H = L.rot ? K : 2 * K;
  return (size_t)(p.tw + 2 * H) * (p.th + 2 * H) * (L.rot ? 6 : 3) * sizeof(double);
}

template <int ROT>
int cool_launch(const SigmaLevel &L, const SmoothPlan &p, uint32_t K, double, uint64_t blocks, const double *src, double *dst, hipStream_t st) {
  const size_t lds = cool_lds(L, p, K);
#define MLMCPI_COOL(NT) \
  hipLaunchKernelGGL((sigma_cool_kernel<ROT, NT>), topo_grid(blocks), dim3(NT), lds, st, L, blocks, src, dst, p.tw, p.th, p.tiles_a, p.tiles, K)
  if (p.nt == 1024) MLMCPI_COOL(1024);
  else if (p.nt == 512) MLMCPI_COOL(512);
  else MLMCPI_COOL(256);
#undef MLMCPI_COOL
  MLMCPI_LAUNCH_CHECK("sigma_cool_kernel");
  return MLMCPI_OK;
}

DeviceOnce g_cool_attr_once;

const Smoother kCooling = {
    "cooling", "cooling", "depth", "depths", MLMCPI_SIGMA_COOLING_MAX_DEPTHS, MLMCPI_SIGMA_COOLING_MAX_DEPTH,
    {&Tuning::sigma_cool_tw, &Tuning::sigma_cool_th, &Tuning::sigma_cool_nt, &Tuning::sigma_cool_fuse}, {32, 32, 512, 2},
    cool_lds, {cool_launch<0>, cool_launch<1>},
    {(const void *)sigma_cool_kernel<0, 256>, (const void *)sigma_cool_kernel<0, 512>, (const void *)sigma_cool_kernel<0, 1024>,
     (const void *)sigma_cool_kernel<1, 256>, (const void *)sigma_cool_kernel<1, 512>, (const void *)sigma_cool_kernel<1, 1024>}, &g_cool_attr_once};

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_sigma_level_cooling_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t n_chains, size_t *bytes) {
  return smooth_workspace_bytes(kCooling, level, n_chains, bytes);
}

int mlmcpi_sigma_level_cooling_plan(const mlmcpi_sigma_level *level, uint32_t n_chains, const uint32_t *depths, uint32_t n_depths,
                                    mlmcpi_sigma_cooling_plan *plan) {
  return smooth_plan_query(kCooling, level, n_chains, depths, n_depths, plan, &mlmcpi_sigma_cooling_plan::launch_sweeps);
}

int mlmcpi_sigma_level_cooled_charge(const mlmcpi_sigma_level *level, const double *d_state, uint32_t n_chains, const uint32_t *depths,
                                     uint32_t n_depths, double *d_q, double *d_chi, double *d_energy, double *d_cooled, void *d_work,
                                     size_t work_bytes, void *stream) {
  return smooth_run(kCooling, level, d_state, n_chains, 0.0, depths, n_depths, d_q, d_chi, d_energy, d_cooled, d_work, work_bytes, stream);
}

}  // extern "C"
