// schwinger_perm.hpp -- K overrelaxation sweeps of the quenched Schwinger model in closed form: the plane of plaquettes in LDS,
// the tasks of a workgroup, the gather (perm_sweeps) and the image its results are laid down as.  Device code of
// schwinger_perm_kernel and schwinger_perm_heat_kernel, for schwinger_sweeps.hip alone: that unit defines and launches both
// kernels (and reads g_stamps, which is defined below: one including unit).
#pragma once
#include "lattice_sweep.hpp"

namespace mlmcpi {

// Instrumentation build only (make EXTRA=-DMLMCPI_STAMPS): thread 0 of every workgroup of
// schwinger_perm_heat_kernel leaves the 100 MHz wall clock at ten points, plus the XCD / CU it ran on.
#ifdef MLMCPI_STAMPS
__device__ unsigned long long g_stamps[16 * 65536];
#define MLMCPI_STAMP(k)                                                                                            \
  do {                                                                                                             \
    if (threadIdx.x == 0 && blockIdx.y * gridDim.x + blockIdx.x < 65536)                                           \
      g_stamps[(blockIdx.y * gridDim.x + blockIdx.x) * 16 + (k)] = __builtin_amdgcn_s_memrealtime();               \
  } while (0)
#define MLMCPI_STAMP_WHERE()                                                                                       \
  do {                                                                                                             \
    if (threadIdx.x == 0 && blockIdx.y * gridDim.x + blockIdx.x < 65536)                                           \
      g_stamps[(blockIdx.y * gridDim.x + blockIdx.x) * 16 + 15] =                                                  \
          ((unsigned long long)__builtin_amdgcn_s_getreg((20 /*XCC_ID*/) | (0 << 6) | (31 << 11)) << 32) |         \
          __builtin_amdgcn_s_getreg((4 /*HW_ID*/) | (0 << 6) | (31 << 11));                                        \
  } while (0)
#else
#define MLMCPI_STAMP(k) do { } while (0)
#define MLMCPI_STAMP_WHERE() do { } while (0)
#endif

// ---- Schwinger overrelaxation in closed form: K sweeps are a fixed permutation of the plaquettes -----------------------
// With P(i, j) = theta_0(i, j) + theta_1(i+1, j) - theta_0(i, j+1) - theta_1(i, j) the two staple sums of the mu = 0 link at
// (i, j) are theta - P(i, j) and theta + P(i, j-1) (quenchedschwingeraction.cc:25-43), so its overrelaxation update
// (quenchedschwingeraction.cc:57-65) is
//     theta <- theta + P(i, j-1) - P(i, j)   (mod 2 pi),
// after which P(i, j) and P(i, j-1) have changed places; likewise theta_1(i, j) <- theta_1 + P(i, j) - P(i-1, j) swaps
// P(i, j) and P(i-1, j).  In the multicolour order of the sweeps here -- (mu = 0, j even), (mu = 0, j odd), (mu = 1, i even),
// (mu = 1, i odd) -- a colour phase therefore swaps whole rows (columns) of plaquettes pairwise, and one sweep moves the
// plaquette at an even row (column) index two rows (columns) down and the one at an odd index two up: after s sweeps
//     P_s(i, j) = P_0(i + 2 s e_i, j + 2 s e_j),   e_x = +1 for even x, -1 for odd x,
// whatever the field is.  Summing the increments of a link over K sweeps gives (s = 0 .. K - 1)
//     theta_0(i, j)  +=  sum_s  P_0(i + 2 s e_i, j - 1 - p_j - 2 s)  -  P_0(i + 2 s e_i, j + p_j + 2 s),        p_x = x mod 2,
//     theta_1(i, j)  +=  sum_s  P_0(i + p_i + 2 s, j + 2 (s + 1) e_j)  -  P_0(i - 1 - p_i - 2 s, j + 2 (s + 1) e_j),
// the same map as K sweeps of any other overrelaxation kernel here up to the rounding of 4 K additions (measured against
// them and against the oracle's sweeps: <= 3e-14 at K = 10).  A link costs 2 K LDS reads and 2 K additions instead of
// 9.3 K fp64 instructions, there is no halo recomputation (only the links that are wanted are computed), no colour
// phases and no barriers between sweeps; what remains is the halo of 2 K in the plaquettes a workgroup needs.
// Pairs: the two mu = 0 links of a column at rows (j, j + 1), j even, share their first stream (p_j cancels in it), and so
// do the two mu = 1 links of a row at columns (i, i + 1), i even, their second: a task is such a pair -- three streams of K
// plaquettes, two links.  With S, X, X' the sums over the shared stream and the two others (each in the order s = 0, 1, ...),
//     mu = 0:  theta_0(i, j) += S - X,  theta_0(i, j+1) += S - X';        mu = 1:  theta_1(i, j) += X - S,  theta_1(i+1, j) += X' - S.
// That order of operations is the definition: a result depends on the field and K only -- not on the tile, the batch, the
// workgroup size or the kernel (schwinger_perm_kernel == the first part of schwinger_perm_heat_kernel, bit for bit) -- but
// K sweeps in one launch and the same sweeps in two differ in the last bits.
//
// The plane: P_0 over `rows` x W vertices in LDS.  A wave takes 63 columns of a group of rows and walks up: lane l loads
// the double2 of column 63 cw + l, row by row -- the load of the next row is the theta_0(i, j+1) of this one, and
// theta_1(i+1, j) comes from lane l + 1 by DPP (lane 63 only serves lane 62): ONE coalesced 16-byte load per plaquette,
// U + 1 rows in flight per thread.  W + 1 <= Mt and rows + 1 <= Mx are not required: columns and rows wrap as often as
// needed (a 64 x 64 lattice is its own halo).
#ifndef MLMCPI_PERM_U
#define MLMCPI_PERM_U 0    // rows in flight per thread in the plane build; 0 = all of a thread's rows at the deepest launch (r05: one round trip to HBM instead of two: -4.2 % on the launch, same-box A/B)
#endif

// The plane in LDS.  Every stream of the closed form walks a diagonal of the plaquettes of ONE parity class: column and
// row parity do not change along it, the column moves by 2 e_c and the row by +-2 per step s.  So the plane is kept as four
// quadrants by (column parity, row parity) with the ODD index mirrored, and -- an even index only grows along a stream, an
// odd one only falls -- each quadrant holds only the columns and rows of its parity that some task reads (PermGeom: the
// read set, col_first .. col_last, row_first .. row_last):
//     column C -> u = (C - col_first(K, 0)) / 2 (C even),  (col_last(K, 1) - C) / 2 (C odd);      row R -> v likewise.
// A step of any stream of any task is then (u, v) -> (u + 1, v + 1): ONE byte stride, kStep, for all of them -- whatever
// the parities, mu = 0 or 1 -- and with the pitch and the quadrant size compile-time constants (the extents of the deepest
// launch, kPermMaxK sweeps; a shallower one leaves columns and rows unused) the K reads of a stream are K immediate
// offsets from one address, and the address of a task's first read does not depend on K: in output coordinates (c, r)
// the read set begins where the tasks do.  (The row-major plane this replaces cost 6.6 integer instructions of address
// arithmetic per read; the four full quadrants of (OW / 2 + 2 K) x (HR / 2 + 2 K) after it held a third more plaquettes than
// anybody reads and did not fit for both halves at once beyond K = 6.)  Same values, same order of additions: results are
// bit for bit those of the row-major form.
template <class PG>
struct PermPlane {
  static constexpr int kRow = PG::kPitch * 8, kStep = kRow + 8;        // bytes
  static constexpr uint32_t QB = (uint32_t)PG::kQRows * kRow;          // bytes per quadrant
  static_assert(kStep == (int)PG::kStep * 8, "the stride of a stream");
  uint32_t K;
  __device__ __forceinline__ explicit PermPlane(uint32_t K_) : K(K_) {}
  // is column C / row R of the plane in the read set?  (C < width(K), R < rows(K))
  __device__ __forceinline__ bool has_col(uint32_t C) const { return (C & 1u) ? C <= PG::col_last(K, 1) : C >= PG::col_first(K, 0) && C <= PG::col_last(K, 0); }
  __device__ __forceinline__ bool has_row(uint32_t R) const { return (R & 1u) ? R <= PG::row_last(K, 1) : R >= PG::row_first(K, 0) && R <= PG::row_last(K, 0); }
  // byte offset of plaquette (C, R) of the read set = col(C) + row(R)
  __device__ __forceinline__ uint32_t col(uint32_t C) const { return (C & 1u) ? QB + PG::col_u(K, C) * 8u : PG::col_u(K, C) * 8u; }
  __device__ __forceinline__ uint32_t row(uint32_t R) const { return (R & 1u) ? 2u * QB + PG::row_v(K, R) * (uint32_t)kRow : PG::row_v(K, R) * (uint32_t)kRow; }
};

// where a thread stands in a build: its theta column, its rows [r, rend) of the `rows`, whether it owns a plaquette column
struct PermBuildPos {
  uint32_t c, r, rend, row_off, gj;   // row_off = gj Mt: the lattice row of build row r, in vertices (< 2^32: check_lattice)
  uint32_t cb;                        // PermPlane::col of the plaquette column
  const double2 *src;                 // the chain (uniform: with the scalar row offset the base of a row's loads) ...
  uint32_t col;                       // ... and the thread's lattice column
  bool active, owns;
};
template <int NT, class PP>
__device__ __forceinline__ PermBuildPos perm_build_pos(const PP &P, const double2 *__restrict__ src, uint32_t Mt, uint32_t Mx, uint32_t gi0,
                                                       uint32_t gj0, uint32_t W, uint32_t rows) {
  PermBuildPos q;
  // (the wave index on the scalar side: rows, row offsets and the loop conditions of the build are then scalar too)
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
  const uint32_t nwc = W > 63 ? 2 : 1;                                // column waves per row group (W <= 108: at most 2)
  const uint32_t groups = (NT / kWave) >> (nwc - 1);                   // row groups
  const uint32_t g = wave >> (nwc - 1), cw = wave & (nwc - 1);
  static_assert(((NT / kWave) & (NT / kWave - 1)) == 0, "waves per workgroup: a power of two (shifts for divisions)");
  const uint32_t rpg = groups == 4 ? (rows + 3) >> 2 : groups == 8 ? (rows + 7) >> 3 : (rows + groups - 1) / groups;
  q.c = 63 * cw + lane;                                                // theta column; the plaquette column of lanes 0 .. 62
  // (rows and row offsets are the same for a whole wave; said so explicitly, so that the conditions on them below are scalar
  // branches: behind a vector condition every load of the chunk waits for the one before it)
  q.r = __builtin_amdgcn_readfirstlane(g * rpg);
  q.rend = __builtin_amdgcn_readfirstlane(g < groups ? min(rows, q.r + rpg) : 0);
  q.active = q.r < q.rend;               // (wave-uniform: not the waves without rows)
  q.owns = lane < 63 && q.c < W && P.has_col(q.c);   // (a wing column is loaded for its neighbour's theta_1 and owns nothing)
  q.cb = P.col(q.c);
  // (the lanes beyond theta column W, which nobody reads, load column W again: a lane condition on the loads would make
  // vector branches of the scalar ones around them, and every load would wait for the one before it)
  q.src = src;
  q.col = wrap_add(gi0, min(q.c, W), Mt);
  q.gj = __builtin_amdgcn_readfirstlane(wrap_add(gj0, q.r, Mx));
  q.row_off = q.gj * Mt;
  return q;
}
// rows (q.r, min(q.r + U, q.rend)] of the thread's column into nxt[0 .. U); first: row q.r itself into cur
template <int U>
__device__ __forceinline__ void perm_rows_load(PermBuildPos &q, uint32_t Mt, uint32_t Mx, bool first, double2 &cur, double2 (&nxt)[U]) {
  if (!q.active) return;
  if (first) cur = (q.src + q.row_off)[q.col];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    q.gj = q.gj + 1 == Mx ? 0 : q.gj + 1;
    q.row_off = q.gj == 0 ? 0 : q.row_off + Mt;
    if (q.r + u < q.rend) nxt[u] = (q.src + q.row_off)[q.col];
  }
}
// their plaquettes into the plane, those of the read set; cur <- the last row, for the next chunk
template <int U, class PP>
__device__ __forceinline__ void perm_rows_store(PermBuildPos &q, const PP &P, double *plane, double2 &cur, const double2 (&nxt)[U]) {
  if (!q.active) return;
  char *const pb = reinterpret_cast<char *>(plane) + q.cb;
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (q.r + u < q.rend) {
      const double right = wave_rotate_down(cur.y);   // theta_1 of the next column
      if (q.owns && P.has_row(q.r + u)) *reinterpret_cast<double *>(pb + P.row(q.r + u)) = ((cur.x + right) - nxt[u].x) - cur.y;   // (the row part is scalar)
      cur = nxt[u];
    }
  q.r += U;
}
// ONCE: U covers a thread's rows at every depth -- no loop, whose back edge would make every load of a chunk wait for the
// loads of the chunk before (their registers are the ones it is about to fill)
template <int NT, int U, bool ONCE, class PP>
__device__ __forceinline__ void perm_build_rows(const PP &P, double *plane, const double2 *__restrict__ src, uint32_t Mt, uint32_t Mx,
                                                uint32_t gi0, uint32_t gj0, uint32_t W, uint32_t rows) {
  PermBuildPos q = perm_build_pos<NT>(P, src, Mt, Mx, gi0, gj0, W, rows);
  double2 cur = make_double2(0., 0.);
  if (ONCE) {
    double2 nxt[U];
    perm_rows_load<U>(q, Mt, Mx, true, cur, nxt);
    perm_rows_store<U>(q, P, plane, cur, nxt);
    return;
  }
  bool first = true;
  while (__builtin_amdgcn_readfirstlane(q.r) < __builtin_amdgcn_readfirstlane(q.rend)) {   // (uniform per wave)
    double2 nxt[U];
    perm_rows_load<U>(q, Mt, Mx, first, cur, nxt);
    perm_rows_store<U>(q, P, plane, cur, nxt);
    first = false;
  }
}

// The tasks of a half and who takes them.  A task is a column pair (mu = 0: rows r, r + 1 of column c) or a row pair
// (mu = 1: columns c, c + 1 of row r), coordinates inside the half.  Whole WAVES take whole rows (r05): a mu = 0 wave-task is
// the mu = 0 tasks of row pair m in columns 0 .. 63 (lane l: the even columns on lanes 0 .. 31, the odd ones on 32 .. 63: a
// 32-lane group of a gather read stays inside one quadrant of the plane, contiguous banks), a mu = 1 wave-task the mu = 1
// tasks of rows 2 m + (l >> 5) in column pairs l & 31; there are H2 = HR / 2 of either kind, m = 0 .. H2 - 1.
// A wave has ONE kind -- the first half of the waves mu = 0, the second mu = 1 -- and wave j of its kind takes a BLOCK of
// consecutive m: Q + 1 = H2 / (NW / 2) + 1 of them for j < R = H2 mod (NW / 2), Q for the others, slot k = the block's k-th.
// So the slots of a mu = 0 thread are consecutive row pairs of ONE column, and the third stream of slot k is the second of
// slot k + 1 -- the same plaquettes in the same order: perm_sweeps sums it once and hands it down the block.
// The kind of a wave and the row of a slot are wave-uniform (scalar), slots 0 .. Q - 1 are full in every wave (known at
// compile time), and the column of a lane is the same in every slot.  The columns beyond 64 of the 68-wide output of the
// fused launch (4 x HR / 2 mu = 0 tasks, 2 x HR mu = 1 tasks) are left-over wave-tasks in the last slot of the waves of
// their kind whose block is the shorter one.  Which lane computes a task does not enter its result.
template <int NT, int RING, int TH = 64>
struct PermTasks {
  using PG = PermGeom<NT, RING, TH>;
  static constexpr int OW = PG::OW, HR = PG::HR, H2 = HR / 2, NW = NT / kWave, NS = PG::NV;
  static constexpr int NWK = NW / 2, Q = H2 / NWK, R = H2 % NWK;      // waves of a kind; the block: Q + 1 (wave j < R of its kind) or Q slots
  static constexpr int XC = OW - 64;                                   // columns beyond a wave's 64 (0 or 4)
  static constexpr int L0 = XC * H2, L1 = (XC / 2) * HR;               // left-over tasks, mu = 0 and mu = 1
  static constexpr int NL0 = (L0 + 63) / 64, NL1 = (L1 + 63) / 64;     // ... as wave-tasks
  static_assert(NW % 2 == 0 && NS == Q + (R > 0 ? 1 : 0), "slots per thread: the longer block");
  static_assert(XC == 0 || (R > 0 && NL0 <= NWK - R && NL1 <= NWK - R), "the left-over wave-tasks fit the free last slots of their kind");
  uint32_t wave, lane, c_mu0, c_mu1, r_lo;
  uint32_t j, m0, len;   // wave j of its kind: the wave-tasks m0 .. m0 + len - 1 (scalar)
  bool kind;             // mu = 1 (scalar)
  __device__ PermTasks() {
    wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    lane = threadIdx.x % kWave;
    c_mu0 = lane < 32 ? 2 * lane : 2 * (lane - 32) + 1;
    c_mu1 = 2 * (lane & 31u);
    r_lo = lane >> 5;
    kind = wave >= (uint32_t)NWK;
    j = kind ? wave - (uint32_t)NWK : wave;
    m0 = j * (uint32_t)Q + min(j, (uint32_t)R);
    len = (uint32_t)Q + (j < (uint32_t)R ? 1u : 0u);
  }
  // f(std::true_type) in the mu = 1 waves, f(std::false_type) in the mu = 0 ones: one scalar branch around all of a wave's slots
  template <class F>
  __device__ __forceinline__ void by_kind(F &&f) const {
    if (kind) f(std::true_type{}); else f(std::false_type{});
  }
  // slot k of the block (0 <= k < NS): is there a wave-task in it?  (k < Q: yes, at compile time)
  __device__ __forceinline__ bool in_block(int k) const { return k < Q || (uint32_t)k < len; }
  // slot k of this thread, a wave of kind MU1: false when there is no task in it
  template <bool MU1>
  __device__ __forceinline__ bool task(int k, uint32_t &r, uint32_t &c) const {
    if (main_task<MU1>(k, r, c)) return true;
    return XC > 0 && k == NS - 1 && left_task<MU1>(r, c);
  }
  // ... when it is one of the block
  template <bool MU1>
  __device__ __forceinline__ bool main_task(int k, uint32_t &r, uint32_t &c) const {
    r = 0; c = 0;
    if (!in_block(k)) return false;
    const uint32_t m = m0 + (uint32_t)k;
    r = MU1 ? 2 * m + r_lo : 2 * m;
    c = MU1 ? c_mu1 : c_mu0;
    return true;
  }
  // the left-over task in slot NS - 1, if the thread has one
  template <bool MU1>
  __device__ __forceinline__ bool left_task(uint32_t &r, uint32_t &c) const {
    r = 0; c = 0;
    if (XC > 0 && !in_block(NS - 1)) {
      const uint32_t jl = j - (uint32_t)R;
      if (!MU1 && jl < (uint32_t)NL0) {                       // mu = 0, columns 64 ..: task L = row pair L / XC, column 64 + L % XC
        const uint32_t L = 64 * jl + lane;
        r = 2 * (L / (XC ? XC : 1));
        c = 64 + L % (XC ? XC : 1);
        return L < (uint32_t)L0;
      }
      if (MU1 && jl < (uint32_t)NL1) {                        // mu = 1, column pairs 32 ..: row L / (XC / 2), column 64 + 2 (L % (XC / 2))
        const uint32_t L = 64 * jl + lane;
        r = L / (XC > 1 ? XC / 2 : 1);
        c = 64 + 2 * (L % (XC > 1 ? XC / 2 : 1));
        return L < (uint32_t)L1;
      }
    }
    return false;
  }
};

// Five steps of the three streams of a task: fifteen 8-byte LDS reads at immediate offsets from three addresses, through
// inline asm (lds_read_f64: the compiler would pair the reads of a stream into ds_read2_b64, half the rate --
// MI355X_MICROARCH.md, LDS table), one wait naming all fifteen, then the additions in the order s = 0, 1, ...
template <int STEP>
__device__ __forceinline__ void perm_gather5(uint32_t pa, uint32_t px, uint32_t px2, double &S, double &X, double &X2) {
  double a0 = lds_read_f64<0>(pa), x0 = lds_read_f64<0>(px), y0 = lds_read_f64<0>(px2);
  double a1 = lds_read_f64<STEP>(pa), x1 = lds_read_f64<STEP>(px), y1 = lds_read_f64<STEP>(px2);
  double a2 = lds_read_f64<2 * STEP>(pa), x2 = lds_read_f64<2 * STEP>(px), y2 = lds_read_f64<2 * STEP>(px2);
  double a3 = lds_read_f64<3 * STEP>(pa), x3 = lds_read_f64<3 * STEP>(px), y3 = lds_read_f64<3 * STEP>(px2);
  double a4 = lds_read_f64<4 * STEP>(pa), x4 = lds_read_f64<4 * STEP>(px), y4 = lds_read_f64<4 * STEP>(px2);
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(a0), "+v"(x0), "+v"(y0), "+v"(a1), "+v"(x1), "+v"(y1), "+v"(a2), "+v"(x2), "+v"(y2), "+v"(a3), "+v"(x3), "+v"(y3),
                 "+v"(a4), "+v"(x4), "+v"(y4)
               :
               : "memory");
  S += a0; X += x0; X2 += y0;
  S += a1; X += x1; X2 += y1;
  S += a2; X += x2; X2 += y2;
  S += a3; X += x3; X2 += y3;
  S += a4; X += x4; X2 += y4;
}
__device__ __forceinline__ void perm_gather1(uint32_t pa, uint32_t px, uint32_t px2, double &S, double &X, double &X2) {
  double a0 = lds_read_f64<0>(pa), x0 = lds_read_f64<0>(px), y0 = lds_read_f64<0>(px2);
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a0), "+v"(x0), "+v"(y0) : : "memory");
  S += a0; X += x0; X2 += y0;
}
// ... and of two streams, for a task whose third one the task before it in the block has summed: ten reads, one wait
template <int STEP>
__device__ __forceinline__ void perm_gather5(uint32_t pa, uint32_t px2, double &S, double &X2) {
  double a0 = lds_read_f64<0>(pa), y0 = lds_read_f64<0>(px2);
  double a1 = lds_read_f64<STEP>(pa), y1 = lds_read_f64<STEP>(px2);
  double a2 = lds_read_f64<2 * STEP>(pa), y2 = lds_read_f64<2 * STEP>(px2);
  double a3 = lds_read_f64<3 * STEP>(pa), y3 = lds_read_f64<3 * STEP>(px2);
  double a4 = lds_read_f64<4 * STEP>(pa), y4 = lds_read_f64<4 * STEP>(px2);
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(a0), "+v"(y0), "+v"(a1), "+v"(y1), "+v"(a2), "+v"(y2), "+v"(a3), "+v"(y3), "+v"(a4), "+v"(y4)
               :
               : "memory");
  S += a0; X2 += y0;
  S += a1; X2 += y1;
  S += a2; X2 += y2;
  S += a3; X2 += y3;
  S += a4; X2 += y4;
}
__device__ __forceinline__ void perm_gather1(uint32_t pa, uint32_t px2, double &S, double &X2) {
  double a0 = lds_read_f64<0>(pa), y0 = lds_read_f64<0>(px2);
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a0), "+v"(y0) : : "memory");
  S += a0; X2 += y0;
}

// res[h][k] = the new angles of the two links of task k of half h
template <int NT, int RING, int TH = 64>
__device__ __forceinline__ void perm_sweeps(double *plane, const double2 *__restrict__ src, uint32_t Mt, uint32_t Mx, uint32_t i0,
                                            uint32_t j0, uint32_t K, double2 (&res)[2][PermGeom<NT, RING, TH>::NV]) {
  using PG = PermGeom<NT, RING, TH>;
  using PP = PermPlane<PG>;
  constexpr int HR = PG::HR, NV = PG::NV;
  // all of a thread's rows at the deepest launch: (2 HR + 4 kPermMaxK) rows over (NT / 64) / 2 row groups (W > 63: two column waves)
  constexpr int kGroups = NT / kWave / 2;
  constexpr int U = MLMCPI_PERM_U ? MLMCPI_PERM_U : (2 * HR + 4 * (int)kPermMaxK + kGroups - 1) / kGroups;   // rows in flight per thread (nothing else is live yet)
  const uint32_t W = PG::width(K), rows = PG::rows(K), H = RING + 2 * K;
  const PP P(K);
  // lattice coordinates of plane (0, 0), and of output vertex (0, 0)
  // (x - h) mod n for x < n: a comparison where h <= n -- the rule; the two modulo operations of the general form are ~80
  // instructions each in front of the first load of the workgroup
  auto back = [](uint32_t x, uint32_t h, uint32_t n) { return h <= n ? (x >= h ? x - h : x + n - h) : (x + n - h % n) % n; };
  const uint32_t gi0 = back(i0, H, Mt), gj0 = back(j0, H, Mx);
  const uint32_t oi0 = back(i0, RING, Mt), oj0 = back(j0, RING, Mx);
  using PT = PermTasks<NT, RING, TH>;
  const PT tasks;
  // the links of a half as they are now (HR, RING, 2 K and the tile origins are even: output parity = plane parity = lattice parity)
  // (32-bit byte offsets from the chain's base pointer -- the host admits lattices of less than 2^28 vertices to these
  // kernels --, wraps by the unsigned-minimum trick: v >= n ? v - n : v = min(v, v - n); twice more for extents below
  // the output window's, a uniform branch.  The 64-bit pointer form this replaces cost 30 vector instructions per task.)
  const char *const src_b = reinterpret_cast<const char *>(src);
  const bool small_lattice = Mx < (uint32_t)(2 * HR + 2) || Mt < (uint32_t)(PG::OW + 2);   // (uniform: two copies of the loop)
  auto load_theta_of = [&](int h, double2 (&th)[NV], auto small, auto kind) {
    constexpr bool MU1 = decltype(kind)::value;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      uint32_t r, c;
      if (!tasks.template task<MU1>(k, r, c)) continue;
      uint32_t gr = oj0 + r + h * HR, gc = oi0 + c;
      gr = min(gr, gr - Mx);
      gc = min(gc, gc - Mt);
      if ((bool)small) {
        gr = min(gr, gr - Mx); gr = min(gr, gr - Mx);
        gc = min(gc, gc - Mt); gc = min(gc, gc - Mt);
      }
      const uint32_t o = (gr * Mt + gc) * 16u;
      if (!MU1) {
        const uint32_t o2 = gr + 1 == Mx ? o - gr * Mt * 16u : o + Mt * 16u;
        th[k] = make_double2(*reinterpret_cast<const double *>(src_b + o), *reinterpret_cast<const double *>(src_b + o2));
      } else {
        const uint32_t o2 = gc + 1 == Mt ? o - gc * 16u : o + 16u;
        th[k] = make_double2(*reinterpret_cast<const double *>(src_b + o + 8u), *reinterpret_cast<const double *>(src_b + o2 + 8u));
      }
    }
  };
  auto load_theta = [&](int h, double2 (&th)[NV], auto kind) {
    if (small_lattice) load_theta_of(h, th, std::true_type{}, kind); else load_theta_of(h, th, std::false_type{}, kind);
  };
  // what K sweeps add to them.  In a mu = 0 wave the third stream of slot k - 1 of the block IS the second of slot k -- the
  // next row pair of the same column: the same address, the same K reads, added in the same order from 0.0 -- so it is
  // summed once, by slot k - 1, and slot k sums two streams: a block of n row pairs costs 2 n + 1 streams, not 3 n.
  auto gather = [&](int h, double2 (&d)[NV], auto kind) {
    constexpr bool MU1 = decltype(kind)::value;
    const uint32_t lds0 = (uint32_t)(uintptr_t)plane;   // the LDS byte address of the plane (lds_read_f64)
    double Xnext = 0.0;                                 // mu = 0: the third stream of the slot before
    // task (r, c) of slot k; chained: its second stream is Xnext
    auto one = [&](int k, uint32_t r, uint32_t c, auto chained_t) {
      constexpr bool chained = decltype(chained_t)::value;
      // the shared stream, the first of the two others and the second, at s = 0 (plane coordinates C = c + 2 K, R = r + h HR + 2 K):
      //   mu = 0 (R even): A_s = P(C + 2 s e_C, R - 1 - 2 s), B_s = P(C + 2 s e_C, R + 2 s), B'_s two rows above B_s;
      //   mu = 1 (C even): D_s = P(C - 1 - 2 s, J_s), J_s = R + 2 (s + 1) e_R, C_s = P(C + 2 s, J_s), C'_s two columns on;
      // in quadrant coordinates every one of them advances by (1, 1) per s, and where it starts does not depend on K: the
      // read set begins at the tasks (PermGeom::col_u, row_v with C = c + 2 K, R = ro + 2 K written out in c and ro)
      const uint32_t ro = r + (uint32_t)(h * HR), cq = c >> 1, rq = ro >> 1;
      uint32_t a, x, x2;
      if (!MU1) {
        const uint32_t cb = (c & 1u) ? PP::QB + ((uint32_t)(PG::OW / 2 - 1) - cq) * 8u : cq * 8u;   // = P.col(C)
        x = cb + rq * (uint32_t)PP::kRow;                                             // row R, even: v = ro / 2
        x2 = x + (uint32_t)PP::kRow;
        a = cb + 2u * PP::QB + ((uint32_t)(HR - 1) - rq) * (uint32_t)PP::kRow;        // row R - 1, odd: v = OH / 2 - 1 - ro / 2
      } else {
        // J_0 = R + 2 (v = ro / 2 + 1) for even R, R - 2 (v = OH / 2 - 1 - (ro - 1) / 2) for odd R
        const uint32_t rb = (ro & 1u) ? 2u * PP::QB + ((uint32_t)(HR - 1) - rq) * (uint32_t)PP::kRow : (rq + 1u) * (uint32_t)PP::kRow;
        x = rb + cq * 8u;                                                             // column C, even: u = c / 2
        x2 = x + 8u;
        a = rb + PP::QB + ((uint32_t)(PG::OW / 2) - cq) * 8u;                         // column C - 1, odd: u = OW / 2 - c / 2
      }
      uint32_t pa = lds0 + a, px = lds0 + x, px2 = lds0 + x2;
      double S = 0.0, X = 0.0, X2 = 0.0;
      uint32_t s = 0;
      if (chained) {
        X = Xnext;
        for (; s + 5 <= K; s += 5) {
          perm_gather5<PP::kStep>(pa, px2, S, X2);
          pa += 5 * PP::kStep;
          px2 += 5 * PP::kStep;
        }
        for (; s < K; ++s) {
          perm_gather1(pa, px2, S, X2);
          pa += PP::kStep;
          px2 += PP::kStep;
        }
      } else {
        for (; s + 5 <= K; s += 5) {
          perm_gather5<PP::kStep>(pa, px, px2, S, X, X2);
          pa += 5 * PP::kStep;
          px += 5 * PP::kStep;
          px2 += 5 * PP::kStep;
        }
        for (; s < K; ++s) {
          perm_gather1(pa, px, px2, S, X, X2);
          pa += PP::kStep;
          px += PP::kStep;
          px2 += PP::kStep;
        }
      }
      Xnext = X2;
      double2 dk = MU1 ? make_double2(X - S, X2 - S) : make_double2(S - X, S - X2);
      // (the differences HERE: moved behind the last task by the scheduler, every task kept three sums live instead of two
      // differences, and the fused launch spilled)
      asm volatile("" : "+v"(dk.x), "+v"(dk.y));
      d[k] = dk;
    };
    // the left-over wave-task first, while few results are live (it takes all three streams), then the block in order
    uint32_t r, c;
    if (PT::XC > 0)
      if (tasks.template left_task<MU1>(r, c)) one(NV - 1, r, c, std::false_type{});
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      if (!tasks.template main_task<MU1>(k, r, c)) continue;   // (scalar; k < Q: at compile time)
      if (!MU1 && k > 0) one(k, r, c, std::true_type{}); else one(k, r, c, std::false_type{});
    }
  };
  auto finish = [&](const double2 (&th)[NV], double2 (&d)[NV], auto kind) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      uint32_t r, c;
      if (tasks.template task<decltype(kind)::value>(k, r, c)) d[k] = make_double2(mod_2pi_fast(th[k].x + d[k].x), mod_2pi_fast(th[k].y + d[k].y));
    }
  };

  perm_build_rows<NT, U, MLMCPI_PERM_U == 0>(P, plane, src, Mt, Mx, gi0, gj0, W, rows);
  // one plane: first half (its angles are in flight across the barrier and the first reads of the plane), second half
  double2 th[NV];
  tasks.by_kind([&](auto kind) { load_theta(0, th, kind); });
  __syncthreads();
  MLMCPI_STAMP(1);  // plane built
  tasks.by_kind([&](auto kind) {
    gather(0, res[0], kind);
    finish(th, res[0], kind);
    MLMCPI_STAMP(2);  // first half gathered
    load_theta(1, th, kind);
    gather(1, res[1], kind);
    finish(th, res[1], kind);
  });
}

// the angles of perm_sweeps into the planes th0, th1 of an OW x 2 HR image (the caller puts barriers around it)
template <int NT, int RING, int TH = 64>
__device__ __forceinline__ void perm_store_image(double *th0, double *th1, const double2 (&res)[2][PermGeom<NT, RING, TH>::NV]) {
  using PG = PermGeom<NT, RING, TH>;
  constexpr int OW = PG::OW, HR = PG::HR, NV = PG::NV;
  const PermTasks<NT, RING, TH> tasks;
  tasks.by_kind([&](auto kind) {
    constexpr bool MU1 = decltype(kind)::value;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        uint32_t r, c;
        if (!tasks.template task<MU1>(k, r, c)) continue;
        const uint32_t o = (r + h * HR) * OW + c;
        if (!MU1) {
          th0[o] = res[h][k].x;
          th0[o + OW] = res[h][k].y;
        } else {
          th1[o] = res[h][k].x;
          th1[o + 1] = res[h][k].y;
        }
      }
  });
}

}  // namespace mlmcpi
