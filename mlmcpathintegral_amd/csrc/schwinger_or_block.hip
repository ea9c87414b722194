// schwinger_or_block.hip -- overrelaxation sweeps of the quenched Schwinger model on 4 x 4 register blocks, with their launcher.
// Nothing is drawn here: the unit includes no sampler (tests/test_csrc_headers.py), so not lattice_sweep.hpp either, which
// declares its two host functions beside the other launchers.
#include "sweep_geometry.hpp"

namespace mlmcpi {

// ---- Schwinger overrelaxation, 4 x 4 register blocks on 64 x 64 tiles (OrBlockGeom, sweep_geometry.hpp) ---------------------
// Measured on MI355X (1024 x 1024, 32 chains; timestamps taken inside the kernel): a sweep costs
// 0.028 ms of the launch, which is the fp64 issue time of its 9 instructions per update, and the rest of the launch
// (0.21 ms at K = 1, against 0.17 ms for a plain copy of the state) is the load and store phase of the workgroups,
// which the two workgroups a CU holds overlap only partly with each other's sweeps.  Persistent workgroups and an
// XCD-aware tile order changed nothing; writing the tile back in whole 1 KiB rows per wave instruction instead of
// 16 B per lane at a 64 B stride took 0.02-0.035 ms off every launch (see the end of the kernel); doing the same for
// the loads did not pay.  The K >= 4 launches run at the package power limit (1.37 kW, sclk 2.17-2.25 GHz).
// The buffer of geometry G (tile + halo G::H) into 4 x 4 register blocks, then KS <= G::H / 2 overrelaxation sweeps on it.
// Ends behind the barrier of the last colour phase: the plane area of the LDS is dead from there on.
template <class G, int KS>
__device__ __forceinline__ void or_block_sweeps(double *lds, const double2 *__restrict__ src, uint32_t Mt, uint32_t Mx,
                                                uint32_t i0, uint32_t j0, double (&t0)[G::PH][G::PW], double (&t1)[G::PH][G::PW]) {
  constexpr int PW = G::PW, PH = G::PH, H = G::H, NPX = G::NPX, NPY = G::NPY, NP = G::NP;
  static_assert(2 * KS <= H, "a sweep costs two sites of halo");
  auto pl = [&](int p) { return lds + p * NP; };
  const uint32_t tid = threadIdx.x;
  if (tid >= (uint32_t)G::NT) {  // waves beyond the blocks (a caller with a wider workgroup): only the barriers
    for (int i = 0; i < 1 + 4 * KS; ++i) __syncthreads();
    return;
  }
  const bool active = tid < NP;
  const int pj = active ? (int)tid / NPX : 0, pi = active ? (int)tid - pj * NPX : 0;
  const int me = active ? (int)tid : 0;  // idle threads of the last wave: every index is entry 0, nothing is written
  // neighbour blocks, clamped into the buffer
  const int dn = pj > 0 ? me - NPX : me, up = pj + 1 < NPY ? me + NPX : me;
  const int lf = pi > 0 ? me - 1 : me, rt = pi + 1 < NPX ? me + 1 : me;
  const int rtdn = (pi + 1 < NPX ? 1 : 0) + (pj > 0 ? -NPX : 0) + me;
  const int lfup = (pi > 0 ? -1 : 0) + (pj + 1 < NPY ? NPX : 0) + me;
  // t0, t1: [c][a] = links of vertex (PW pi + a, PH pj + c)

  // the block's columns in the lattice: H is even, so (gi, gi + 1) never straddles the wrap, (gi + 1, gi + 2) may
  {
    uint32_t gi[PW / 2], gj[PH];
    gi[0] = (uint32_t)(((uint64_t)i0 + Mt - (H % Mt) + PW * pi) % Mt);
    gj[0] = (uint32_t)(((uint64_t)j0 + Mx - (H % Mx) + PH * pj) % Mx);
#pragma unroll
    for (int a = 1; a < PW / 2; ++a) gi[a] = gi[a - 1] + 2 == Mt ? 0 : gi[a - 1] + 2;
#pragma unroll
    for (int c = 1; c < PH; ++c) gj[c] = gj[c - 1] + 1 == Mx ? 0 : gj[c - 1] + 1;
#pragma unroll
    for (int c = 0; c < PH; ++c)
#pragma unroll
      for (int a = 0; a < PW; a += 2) {
        double2 v0 = make_double2(0, 0), v1 = v0;
        if (active) {
          v0 = src[(size_t)gj[c] * Mt + gi[a / 2]];
          v1 = src[(size_t)gj[c] * Mt + gi[a / 2] + 1];
        }
        t0[c][a] = v0.x; t1[c][a] = v0.y; t0[c][a + 1] = v1.x; t1[c][a + 1] = v1.y;
      }
  }
  // what a neighbour reads of link mu at (a, c): up to three lists, a corner value once
  auto publish = [&](int mu, int a, int c, double v) {
    const int p1 = c == PH - 1 ? (mu ? G::top1(a) : G::top0(a)) : -1;
    const int p2 = mu == 0 ? (c == 0 ? G::bot0(a) : -1) : (a == 0 ? G::left1(c) : -1);
    const int p3 = a == PW - 1 ? (mu ? G::right1(c) : G::right0(c)) : -1;
    if (!active) return;
    if (p1 >= 0) pl(p1)[me] = v;
    if (p2 >= 0 && p2 != p1) pl(p2)[me] = v;
    if (p3 >= 0 && p3 != p1 && p3 != p2) pl(p3)[me] = v;
  };
#pragma unroll
  for (int c = 0; c < PH; ++c)
#pragma unroll
    for (int a = 0; a < PW; ++a) {
      publish(0, a, c, t0[c][a]);
      publish(1, a, c, t1[c][a]);
    }
  __syncthreads();

  for (int s = 0; s < KS; ++s) {
    // row -1: t0(a, -1), t1(a, -1) for a = 0 .. PW (the last from the block below to the right);
    // column PW: t1(PW, c) for c = -1 .. PH - 1 at index c + 1.  None of these changes during phases 0 and 1.
    double dn0[PW], dn1[PW + 1], rt1[PH + 1];
#pragma unroll
    for (int a = 0; a < PW; ++a) {
      dn0[a] = pl(G::top0(a))[dn];
      dn1[a] = pl(G::top1(a))[dn];
    }
    dn1[PW] = pl(G::top1(0))[rtdn];
    rt1[0] = dn1[PW];
#pragma unroll
    for (int c = 0; c < PH; ++c) rt1[c + 1] = pl(G::left1(c))[rt];
    // phases 0, 1: mu = 0, even rows then odd rows
    //   tp = t0(i, j+1) + t1(i, j) - t1(i+1, j),  tm = t0(i, j-1) + t1(i+1, j-1) - t1(i, j-1)
    double up0[PW + 1];  // row PH: t0(a, PH) for a = -1 .. PW - 1 at index a + 1 (final after phase 0)
#pragma unroll
    for (int par = 0; par < 2; ++par) {
      if (par == 1) {
#pragma unroll
        for (int a = 0; a < PW; ++a) up0[a + 1] = pl(G::bot0(a))[up];
        up0[0] = pl(G::bot0(PW - 1))[lfup];
      }
#pragma unroll
      for (int c = par; c < PH; c += 2)
#pragma unroll
        for (int a = 0; a < PW; ++a) {
          const double t0_up = c + 1 < PH ? t0[c + 1 < PH ? c + 1 : 0][a] : up0[a + 1];
          const double t0_dn = c > 0 ? t0[c > 0 ? c - 1 : 0][a] : dn0[a];
          const double t1_c = t1[c][a];
          const double t1_r = a + 1 < PW ? t1[c][a + 1 < PW ? a + 1 : 0] : rt1[c + 1];
          const double t1_dr = c > 0 ? (a + 1 < PW ? t1[c > 0 ? c - 1 : 0][a + 1 < PW ? a + 1 : 0] : rt1[c]) : dn1[a + 1];
          const double t1_dc = c > 0 ? t1[c > 0 ? c - 1 : 0][a] : dn1[a];
          const double tp = t0_up + t1_c - t1_r;
          const double tm = t0_dn + t1_dr - t1_dc;
          t0[c][a] = mod_2pi_fast((tp + tm) - t0[c][a]);
          publish(0, a, c, t0[c][a]);
        }
      __syncthreads();
    }
    // column -1: t0(-1, c) for c = 0 .. PH (the last is up0[0]), t1(-1, c); final after phase 1
    double lf0[PH + 1], lf1[PH];
#pragma unroll
    for (int c = 0; c < PH; ++c) {
      lf0[c] = pl(G::right0(c))[lf];
      lf1[c] = pl(G::right1(c))[lf];
    }
    lf0[PH] = up0[0];
    // phases 2, 3: mu = 1, even columns then odd columns
    //   tp = t0(i, j) + t1(i+1, j) - t0(i, j+1),  tm = t0(i-1, j+1) + t1(i-1, j) - t0(i-1, j)
#pragma unroll
    for (int par = 0; par < 2; ++par) {
      if (par == 1) {  // the right neighbour's column 0 changed in phase 2
#pragma unroll
        for (int c = 0; c < PH; ++c) rt1[c + 1] = pl(G::left1(c))[rt];
      }
#pragma unroll
      for (int a = par; a < PW; a += 2)
#pragma unroll
        for (int c = 0; c < PH; ++c) {
          const double t0_c = t0[c][a];
          const double t1_r = a + 1 < PW ? t1[c][a + 1 < PW ? a + 1 : 0] : rt1[c + 1];
          const double t0_u = c + 1 < PH ? t0[c + 1 < PH ? c + 1 : 0][a] : up0[a + 1];
          const double t0_lu = a > 0 ? (c + 1 < PH ? t0[c + 1 < PH ? c + 1 : 0][a > 0 ? a - 1 : 0] : up0[a]) : lf0[c + 1];
          const double t1_l = a > 0 ? t1[c][a > 0 ? a - 1 : 0] : lf1[c];
          const double t0_l = a > 0 ? t0[c][a > 0 ? a - 1 : 0] : lf0[c];
          const double tp = t0_c + t1_r - t0_u;
          const double tm = t0_lu + t1_l - t0_l;
          t1[c][a] = mod_2pi_fast((tp + tm) - t1[c][a]);
          publish(1, a, c, t1[c][a]);
        }
      __syncthreads();
    }
  }
}

template <int K>
__global__ void __launch_bounds__(OrBlockGeom<K>::NT)
    schwinger_or_block_kernel(uint32_t Mt, uint32_t Mx, const double2 *__restrict__ in, double2 *__restrict__ out,
                              uint32_t tiles_x) {
  using G = OrBlockGeom<K>;
  constexpr int TW = G::TW, TH = G::TH, PW = G::PW, PH = G::PH, H = G::H, NPX = G::NPX, NP = G::NP;
  extern __shared__ double lds[];
  const uint32_t tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const uint32_t i0 = tx * TW, j0 = ty * TH;
  double t0[PH][PW], t1[PH][PW];
  or_block_sweeps<G, K>(lds, in + (size_t)b * Mt * Mx, Mt, Mx, i0, j0, t0, t1);

  // Owned vertices: buffer columns [H, H + TW), rows [H, H + TH).  A thread holds PW consecutive vertices of a row
  // (64 B), so storing block-wise would make every wave instruction write 64 x 16 B at a 64 B stride.  Instead each wave
  // transposes through LDS (the plane area is dead after the last barrier; wave-private staging, no workgroup barrier):
  // per block row c the owners put their four vertices down, and the wave writes the 256 vertices back as 4 coalesced
  // instructions -- lane l takes vertex l & 3 of block 16 i + (l >> 2), i = 0 .. 3.
  static_assert(PW == 4, "the coalesced side moves 4 vertices per block row");
  const uint32_t wave0 = tid & ~63u, lane = tid & 63u;
  double2 *stage = reinterpret_cast<double2 *>(lds) + (wave0 / 64) * (64 * PW);
  double2 *dst = out + (size_t)b * Mt * Mx;
  int uq[4], ur[4];  // tile coordinates of the vertex this lane writes for i = 0 .. 3 (row c = 0); uq < 0: none
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int bt = (int)wave0 + 16 * i + (int)(lane >> 2);
    const int bj = bt / NPX, bi = bt - bj * NPX;
    uq[i] = PW * bi + (int)(lane & 3) - H;
    ur[i] = PH * bj - H;
    if (bt >= NP || uq[i] >= TW) uq[i] = -1;
  }
#pragma unroll
  for (int c = 0; c < PH; ++c) {
#pragma unroll
    for (int a = 0; a < PW; ++a) stage[PW * lane + a] = make_double2(t0[c][a], t1[c][a]);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double2 w = stage[64 * i + lane];
      const int r = ur[i] + c;
      // (non-temporal, r05: one sweep 0.231 -> 0.226 ms over three same-box pairs)
      if (uq[i] >= 0 && r >= 0 && r < TH) store_streaming(&dst[(size_t)(j0 + r) * Mt + (i0 + uq[i])], w.x, w.y);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// schwinger_or_block_kernel: the depth is the launch's overrelaxation count
int schwinger_or_block_launch(const SweepLaunch &l, const SweepArgs &a) {
  const dim3 grid(l.grid_x, a.B);
  return with_depth<6>(l.n_overrelax, [&](auto kc) -> int {
    constexpr int K = decltype(kc)::value;
    hipLaunchKernelGGL(schwinger_or_block_kernel<K>, grid, dim3(l.threads), l.lds_bytes, a.st, a.Mt, a.Mx, (const double2 *)a.src,
                       (double2 *)a.dst, l.tiles_x);
    MLMCPI_LAUNCH_CHECK("register-block overrelaxation kernel");
    return MLMCPI_OK;
  });
}

// kernels whose LDS may exceed the 64 KiB default
int schwinger_or_block_allow_lds() {
  if (int rc = allow_lds((const void *)schwinger_or_block_kernel<5>, OrBlockGeom<5>::lds_bytes)) return rc;
  if (int rc = allow_lds((const void *)schwinger_or_block_kernel<6>, OrBlockGeom<6>::lds_bytes)) return rc;
  return MLMCPI_OK;
}

}  // namespace mlmcpi
