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
// Launches of a call:
//   1. sigma_cool_stage_kernel: sigma_of(angles) -> buffer A, one sincos pair per vertex (depth 0).
//   2. sigma_cool_kernel<ROT, NT>: one workgroup per tile per chain loads TW x TH vertices (rotated: plane cells, E and O) plus the
//      halo K fused sweeps need (plain 2 K vertices, sigma2d.hip; rotated K cells, sigma_levels.hip) from one buffer, runs K sweeps
//      in LDS, one barrier per phase, each phase on exactly the sites whose inputs are still exact, and writes the tile to the other
//      buffer.  K <= the plan's fuse depth and a launch never runs past the next listed depth.  Tiles that do not divide the plane
//      and halos that pass its edge wrap with modular loads.
//   3. at each listed depth: sigma_cool_charge_kernel<ROT> -- the tile, staging, faces and sum order of sigma_topo_tile_kernel
//      (sigma_topology_device.hpp), fed from the vector buffer --, sigma_cool_energy_kernel<ROT> -- sigma_l . Delta_l summed per
//      group of 256 consecutive vertices (block_sum) -- and sigma_cool_finish_kernel, one workgroup per chain (chain_sum of both).
//   4. sigma_cool_angles_kernel with d_cooled.
// An update is a pure function of four stored vectors, so a halo vertex recomputed by a neighbouring tile gets the bits its owner
// computes, and a vertex written to the buffer and loaded again is the vertex that stayed in LDS: the field of depth d does not
// depend on the tile, the workgroup size, the fuse depth or the depths listed before d.  The sums are functions of the level alone.
// No atomics; workgroups of every launch ride one linear index over grid x and then y (topo_grid).
#include "internal.hpp"

#include "sigma_field_device.hpp"  // the field's layout and the face code; fp contraction is off from here on

namespace mlmcpi {

__device__ __forceinline__ V3 sigma_cool(const V3 &sig, const V3 &Dl) {
  const double n2 = (Dl.x * Dl.x + Dl.y * Dl.y) + Dl.z * Dl.z;
  if (!(n2 > 0.0)) return sig;
  const double nrm = sqrt(n2);
  return V3{Dl.x / nrm, Dl.y / nrm, Dl.z / nrm};
}

// workgroup (chain, group g of 256 vertices): depth 0 of the field
__global__ void __launch_bounds__(kGroup)
    sigma_cool_stage_kernel(uint32_t n, uint32_t ngroups, uint64_t nblocks, const double2 *__restrict__ phi, double *__restrict__ vec) {
  const uint64_t wg = topo_block();
  if (wg >= nblocks) return;
  const uint64_t b = wg / ngroups;
  const uint32_t l = (uint32_t)(wg % ngroups) * kGroup + threadIdx.x;
  if (l < n) cool_store(vec + b * 3 * n, n, l, sigma_of(phi[b * n + l]));
}

// the same map back: the angles of the field
__global__ void __launch_bounds__(kGroup)
    sigma_cool_angles_kernel(uint32_t n, uint32_t ngroups, uint64_t nblocks, const double *__restrict__ vec, double2 *__restrict__ phi) {
  const uint64_t wg = topo_block();
  if (wg >= nblocks) return;
  const uint64_t b = wg / ngroups;
  const uint32_t l = (uint32_t)(wg % ngroups) * kGroup + threadIdx.x;
  if (l < n) phi[b * n + l] = angles_of(cool_fetch(vec + b * 3 * n, n, l));
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
    const V3 e = cool_fetch(s, n, l);
    lds[c] = e.x;
    lds[P + c] = e.y;
    lds[2 * P + c] = e.z;
    if constexpr (ROT) {
      const V3 o = cool_fetch(s, n, L.q + l);
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
            cool_store(d, n, p * L.q + ((sb + lb) % L.hx) * L.ht + (sa + la) % L.ht, v);
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
            cool_store(d, n, (size_t)((sb + lb) % L.Mx) * L.Mt + (sa + la) % L.Mt, v);
        }
      }
      __syncthreads();
    }
  }
}

// ---- measurement at a listed depth ------------------------------------------------------------------------------------------
// sigma_topo_tile_kernel on the vector buffer: partial[chain][tile]
template <int ROT>
__global__ void __launch_bounds__(kTopoThreads)
    sigma_cool_charge_kernel(TopoPlan G, uint64_t nblocks, const double *__restrict__ vec, double *__restrict__ partial) {
  constexpr uint32_t NP = ROT ? 2 : 1;
  __shared__ double sig[NP * 3 * kTopoPlane];
  __shared__ double red[kTopoThreads / kWave];
  const uint64_t wg = topo_block();
  if (wg >= nblocks) return;
  const TopoTile T = topo_tile(G, (uint32_t)(wg % G.tiles));
  const double *s = vec + (wg / G.tiles) * 3 * G.nvert;
  const uint32_t n = G.nvert;

  topo_stage<ROT>(G, T, sig, [s, n](size_t l) { return cool_fetch(s, n, l); });
  __syncthreads();

  double acc[1] = {topo_faces<ROT>(T, sig)};
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) partial[wg] = acc[0];
}

// workgroup (chain, group g): sum over the vertices l of the group of sigma_l . Delta_l -> partial[chain][g]
template <int ROT>
__global__ void __launch_bounds__(kGroup)
    sigma_cool_energy_kernel(SigmaLevel L, uint32_t ngroups, uint64_t nblocks, const double *__restrict__ vec, double *__restrict__ partial) {
  __shared__ double red[kGroup / kWave];
  const uint64_t wg = topo_block();
  if (wg >= nblocks) return;
  const uint32_t n = L.nvert(), l = (uint32_t)(wg % ngroups) * kGroup + threadIdx.x;
  const double *s = vec + (wg / ngroups) * 3 * n;
  double acc[1] = {0.0};
  if (l < n) {
    uint32_t nb[4];
    if constexpr (ROT) {
      const uint32_t p = l >= L.q ? 1 : 0, r = l - p * L.q, a = r % L.ht, b = r / L.ht;
      if (p) {  // O(a, b): E(a+1, b+1), E(a+1, b), E(a, b+1), E(a, b)
        const uint32_t ap = a + 1 == L.ht ? 0 : a + 1, bp = b + 1 == L.hx ? 0 : b + 1;
        nb[0] = bp * L.ht + ap;
        nb[1] = b * L.ht + ap;
        nb[2] = bp * L.ht + a;
        nb[3] = b * L.ht + a;
      } else {  // E(a, b): O(a, b), O(a, b-1), O(a-1, b), O(a-1, b-1)
        const uint32_t am = a == 0 ? L.ht - 1 : a - 1, bm = b == 0 ? L.hx - 1 : b - 1;
        nb[0] = L.q + b * L.ht + a;
        nb[1] = L.q + bm * L.ht + a;
        nb[2] = L.q + b * L.ht + am;
        nb[3] = L.q + bm * L.ht + am;
      }
    } else {
      const uint32_t i = l % L.Mt, j = l / L.Mt;
      nb[0] = j * L.Mt + (i + 1 == L.Mt ? 0 : i + 1);
      nb[1] = j * L.Mt + (i == 0 ? L.Mt - 1 : i - 1);
      nb[2] = (j + 1 == L.Mx ? 0 : j + 1) * L.Mt + i;
      nb[3] = (j == 0 ? L.Mx - 1 : j - 1) * L.Mt + i;
    }
    acc[0] = dot3(cool_fetch(s, n, l), add4(cool_fetch(s, n, nb[0]), cool_fetch(s, n, nb[1]), cool_fetch(s, n, nb[2]), cool_fetch(s, n, nb[3])));
  }
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) partial[wg] = acc[0];
}

// workgroup b < n_chains, column k of the outputs: Q = sum of the tile partials / 2 pi, chi = Q^2 / n, E = 2 n - sum of the
// group partials / 2
__global__ void __launch_bounds__(kGroup)
    sigma_cool_finish_kernel(const double *__restrict__ part_q, uint32_t tiles, const double *__restrict__ part_e, uint32_t ngroups,
                             uint64_t n_chains, double n, uint32_t n_depths, uint32_t k, double *__restrict__ q, double *__restrict__ chi,
                             double *__restrict__ energy) {
  __shared__ double red[kGroup / kWave];
  const uint64_t b = topo_block();
  if (b >= n_chains) return;
  double v[1];
  if (q || chi) {
    chain_sum<1>(part_q + b * tiles, tiles, v, red);
    if (threadIdx.x == 0) {
      const double Q = v[0] / kTwoPi;
      if (q) q[b * n_depths + k] = Q;
      if (chi) chi[b * n_depths + k] = (Q * Q) / n;
    }
  }
  if (energy) {
    __syncthreads();  // red is used again
    chain_sum<1>(part_e + b * ngroups, ngroups, v, red);
    if (threadIdx.x == 0) energy[b * n_depths + k] = 2.0 * n - 0.5 * v[0];
  }
}

// ---- what the gradient flow shares (sigma_field_device.hpp) ---------------------------------------------------------------------
CoolWork cool_work(const SigmaLevel &L, uint32_t n_chains) {
  CoolWork w;
  w.ngroups = (L.nvert() + kGroup - 1) / kGroup;
  w.vec = align256((size_t)n_chains * 3 * L.nvert() * sizeof(double));
  w.part_q = align256((size_t)n_chains * topo_plan(L).tiles * sizeof(double));
  w.part_e = align256((size_t)n_chains * w.ngroups * sizeof(double));
  w.total = 2 * w.vec + w.part_q + w.part_e;
  return w;
}

int cool_stage(const SigmaLevel &L, const CoolWork &w, uint32_t n_chains, const double *d_state, double *vec, hipStream_t st) {
  const uint64_t vblocks = (uint64_t)n_chains * w.ngroups;
  hipLaunchKernelGGL(sigma_cool_stage_kernel, topo_grid(vblocks), dim3(kGroup), 0, st, L.nvert(), w.ngroups, vblocks, (const double2 *)d_state, vec);
  MLMCPI_LAUNCH_CHECK("sigma_cool_stage_kernel");
  return MLMCPI_OK;
}

int cool_measure(const SigmaLevel &L, const CoolWork &w, uint32_t n_chains, const double *vec, double *part_q, double *part_e,
                 uint32_t n_cols, uint32_t k, double *d_q, double *d_chi, double *d_energy, hipStream_t st) {
  const TopoPlan G = topo_plan(L);
  const uint64_t vblocks = (uint64_t)n_chains * w.ngroups, qblocks = (uint64_t)n_chains * G.tiles;
  if (d_q || d_chi) {
    if (L.rot) hipLaunchKernelGGL(sigma_cool_charge_kernel<1>, topo_grid(qblocks), dim3(kTopoThreads), 0, st, G, qblocks, vec, part_q);
    else hipLaunchKernelGGL(sigma_cool_charge_kernel<0>, topo_grid(qblocks), dim3(kTopoThreads), 0, st, G, qblocks, vec, part_q);
    MLMCPI_LAUNCH_CHECK("sigma_cool_charge_kernel");
  }
  if (d_energy) {
    if (L.rot) hipLaunchKernelGGL(sigma_cool_energy_kernel<1>, topo_grid(vblocks), dim3(kGroup), 0, st, L, w.ngroups, vblocks, vec, part_e);
    else hipLaunchKernelGGL(sigma_cool_energy_kernel<0>, topo_grid(vblocks), dim3(kGroup), 0, st, L, w.ngroups, vblocks, vec, part_e);
    MLMCPI_LAUNCH_CHECK("sigma_cool_energy_kernel");
  }
  hipLaunchKernelGGL(sigma_cool_finish_kernel, topo_grid(n_chains), dim3(kGroup), 0, st, (const double *)part_q, G.tiles, (const double *)part_e,
                     w.ngroups, (uint64_t)n_chains, (double)L.nvert(), n_cols, k, d_q, d_chi, d_energy);
  MLMCPI_LAUNCH_CHECK("sigma_cool_finish_kernel");
  return MLMCPI_OK;
}

int cool_angles(const SigmaLevel &L, const CoolWork &w, uint32_t n_chains, const double *vec, double *d_out, hipStream_t st) {
  const uint64_t vblocks = (uint64_t)n_chains * w.ngroups;
  hipLaunchKernelGGL(sigma_cool_angles_kernel, topo_grid(vblocks), dim3(kGroup), 0, st, L.nvert(), w.ngroups, vblocks, vec, (double2 *)d_out);
  MLMCPI_LAUNCH_CHECK("sigma_cool_angles_kernel");
  return MLMCPI_OK;
}

namespace {

struct CoolPlan {
  uint32_t tw, th, nt, fuse, tiles_a, tiles;
};

// Tile, workgroup size and fuse depth: the option, else 32 x 32 (vertices or cells), 512 threads, two sweeps per launch (DESIGN.md
// 4.1g: 38 KB of LDS on a plain level, 62 KB on a rotated one); the tile never exceeds the plane.
CoolPlan cool_plan(const SigmaLevel &L, const Tuning &t) {
  CoolPlan p{t.sigma_cool_tw ? t.sigma_cool_tw : 32u, t.sigma_cool_th ? t.sigma_cool_th : 32u, t.sigma_cool_nt ? t.sigma_cool_nt : 512u,
             t.sigma_cool_fuse ? t.sigma_cool_fuse : 2u, 0, 0};
  const uint32_t PW = L.rot ? L.ht : L.Mt, PH = L.rot ? L.hx : L.Mx;
  if (p.tw > PW) p.tw = PW;
  if (p.th > PH) p.th = PH;
  p.tiles_a = (PW + p.tw - 1) / p.tw;
  p.tiles = p.tiles_a * ((PH + p.th - 1) / p.th);
  return p;
}

inline size_t cool_lds(const SigmaLevel &L, const CoolPlan &p, uint32_t K) {
  const uint32_t H = L.rot ? K : 2 * K;
  return (size_t)(p.tw + 2 * H) * (p.th + 2 * H) * (L.rot ? 6 : 3) * sizeof(double);
}

// what the call and its plan query refuse alike; the plan (one snapshot of the knobs per call) comes back through `plan`.  Its LDS
// image fits: the option table takes no plan whose images do not, and cool_plan only shrinks tiles.
int cool_check(const mlmcpi_sigma_level *level, uint32_t n_chains, const uint32_t *depths, uint32_t n_depths, CoolPlan *plan) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(n_chains > 0, "cooling needs n_chains > 0");
  MLMCPI_REQUIRE(depths, "cooling needs a list of depths (depths is NULL)");
  MLMCPI_REQUIRE(n_depths >= 1 && n_depths <= MLMCPI_SIGMA_COOLING_MAX_DEPTHS, "cooling takes 1 .. %d depths (got %u)",
                 MLMCPI_SIGMA_COOLING_MAX_DEPTHS, n_depths);
  for (uint32_t k = 0; k < n_depths; ++k) {
    MLMCPI_REQUIRE(k == 0 || depths[k] > depths[k - 1], "the cooling depths must be strictly ascending (depths[%u] = %u after %u)", k,
                   depths[k], k ? depths[k - 1] : 0);
    MLMCPI_REQUIRE(depths[k] <= MLMCPI_SIGMA_COOLING_MAX_DEPTH, "a cooling depth is at most %d (depths[%u] = %u)",
                   MLMCPI_SIGMA_COOLING_MAX_DEPTH, k, depths[k]);
  }
  const SigmaLevel L = make_level(*level);
  const CoolPlan p = *plan = cool_plan(L, tuning());
  const uint64_t most = (uint64_t)n_chains * (p.tiles > (L.nvert() + kGroup - 1) / kGroup ? p.tiles : (L.nvert() + kGroup - 1) / kGroup);
  MLMCPI_REQUIRE(most <= kTopoMaxBlocks, "cooling takes at most %llu workgroups per launch (these chains need %llu)",
                 (unsigned long long)kTopoMaxBlocks, (unsigned long long)most);
  return MLMCPI_OK;
}

DeviceOnce g_cool_attr_once;

int cool_init_kernels() {  // the cooling kernel may take the whole LDS (of the current device)
  return once_per_device(g_cool_attr_once, []() -> int {
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_cool_kernel<0, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_cool_kernel<0, 512>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_cool_kernel<0, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_cool_kernel<1, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_cool_kernel<1, 512>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_cool_kernel<1, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, kSigmaLdsMax));
    return MLMCPI_OK;
  });
}

template <int ROT>
int cool_launch(const SigmaLevel &L, const CoolPlan &p, uint32_t K, uint64_t blocks, const double *src, double *dst, hipStream_t st) {
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

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_sigma_level_cooling_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t n_chains, size_t *bytes) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(bytes, "the cooling workspace query needs somewhere to write (bytes is NULL)");
  MLMCPI_REQUIRE(n_chains > 0, "cooling needs n_chains > 0");
  *bytes = cool_work(make_level(*level), n_chains).total;
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_cooling_plan(const mlmcpi_sigma_level *level, uint32_t n_chains, const uint32_t *depths, uint32_t n_depths,
                                    mlmcpi_sigma_cooling_plan *plan) {
  MLMCPI_REQUIRE(plan, "the cooling plan query needs somewhere to write (plan is NULL)");
  CoolPlan p;
  if (int rc = cool_check(level, n_chains, depths, n_depths, &p)) return rc;
  const SigmaLevel L = make_level(*level);
  *plan = mlmcpi_sigma_cooling_plan{};
  plan->tw = p.tw;
  plan->th = p.th;
  plan->nt = p.nt;
  plan->fuse = p.fuse;
  plan->tiles = p.tiles;
  plan->n_measurements = n_depths;
  uint32_t done = 0, deepest = 0;
  for (uint32_t k = 0; k < n_depths; ++k)
    while (done < depths[k]) {
      const uint32_t K = depths[k] - done < p.fuse ? depths[k] - done : p.fuse;
      plan->launch_sweeps[plan->n_launches++] = (uint8_t)K;
      if (K > deepest) deepest = K;
      done += K;
    }
  plan->lds_bytes = deepest ? (uint32_t)cool_lds(L, p, deepest) : 0;
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_cooled_charge(const mlmcpi_sigma_level *level, const double *d_state, uint32_t n_chains, const uint32_t *depths,
                                     uint32_t n_depths, double *d_q, double *d_chi, double *d_energy, double *d_cooled, void *d_work,
                                     size_t work_bytes, void *stream) {
  CoolPlan p;
  if (int rc = cool_check(level, n_chains, depths, n_depths, &p)) return rc;
  MLMCPI_REQUIRE(d_state, "cooling needs a state (d_state is NULL)");
  MLMCPI_REQUIRE(d_q || d_chi || d_energy, "cooling needs d_q, d_chi or d_energy (all three are NULL)");
  MLMCPI_REQUIRE(d_work, "cooling needs its workspace (d_work is NULL)");
  const SigmaLevel L = make_level(*level);
  const CoolWork w = cool_work(L, n_chains);
  MLMCPI_REQUIRE(work_bytes >= w.total, "the cooling workspace is too small: %zu bytes given, %zu needed", work_bytes, w.total);
  if (int rc = cool_init_kernels()) return rc;
  hipStream_t st = as_stream(stream);
  double *cur = (double *)d_work, *other = (double *)((char *)d_work + w.vec);
  double *part_q = (double *)((char *)d_work + 2 * w.vec), *part_e = (double *)((char *)d_work + 2 * w.vec + w.part_q);
  const uint64_t cblocks = (uint64_t)n_chains * p.tiles;

  if (int rc = cool_stage(L, w, n_chains, d_state, cur, st)) return rc;
  uint32_t done = 0;
  for (uint32_t k = 0; k < n_depths; ++k) {
    while (done < depths[k]) {
      const uint32_t K = depths[k] - done < p.fuse ? depths[k] - done : p.fuse;
      if (int rc = L.rot ? cool_launch<1>(L, p, K, cblocks, cur, other, st) : cool_launch<0>(L, p, K, cblocks, cur, other, st)) return rc;
      double *t = cur;
      cur = other;
      other = t;
      done += K;
    }
    if (int rc = cool_measure(L, w, n_chains, cur, part_q, part_e, n_depths, k, d_q, d_chi, d_energy, st)) return rc;
  }
  if (d_cooled)
    if (int rc = cool_angles(L, w, n_chains, cur, d_cooled, st)) return rc;
  return MLMCPI_OK;
}

}  // extern "C"
