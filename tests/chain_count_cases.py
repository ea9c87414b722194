"""Case table of tests/test_chain_count_gpu.py: every batched entry point of include/mlmcpi_hip.h at the 65535-chain edge of the
launch grid.  Everything here is decided without a device; tests/test_chain_count_cases.py asserts the table's own conditions
(every export with a `uint32_t B` is covered or excluded by name, partial last workgroups, the memory cap).

What the runtime does with gridDim.y > 65535 was measured once through mlmcpi_path_initialise (DESIGN.md "Chains per call"): it
launches, and every chain is right.  So Y_ABOVE = "takes": the unguarded entry points are run above the edge, the four units
that refuse by name (rotor_sweeps.hip, sigma_levels.hip, sigma_twolevel.hip, sigma_correlator.hip) keep their guards and their
own refusal tests, and are run here at B_EDGE only.

A case = one call sequence through the ABI at the smallest shape the entry point takes:
  op        the runner of tests/test_chain_count_gpu.py (RUNNERS[op])
  shape     its keyword arguments
  symbols   the exports it calls with the batch size
  kind      "map" (deterministic: long-double reference on every chain) or "draw" (oracle / restatement on the pinned chains)
  rides     where the chains ride in the launches it reaches: "y", "z", "y/16", "x" (one workgroup per chain), "x/4" .. "x/256"
            (packed), "linear" (chains times tiles over one workgroup index)
  above     "takes" or "refuses" above B_EDGE
  split     how the batch compares with the same chains run as two calls: "bits" where the header promises independence from
            the batch split or the plan is the same for both sizes and the kernel has a fixed summation order, else the entry
            point's tolerance
  doubles   doubles per chain the test holds on the device (inputs, outputs, their guarded copies, the split re-run)
  work      bytes of library workspace per chain (from the header's formulas, rounded up)
"""
import collections
import functools

import numpy as np

from lattice_reference import LD, PI, mod_2pi

B_EDGE = 65535                 # the largest batch every entry point takes
B_BIG = 65581                  # past the edge, and a partial last workgroup for every packing (mod 4, 16, 64, 256 != 0)
SPLIT = 40000                  # the uneven point of the two-call run
PACKINGS = (4, 16, 64, 256)
Y_ABOVE = "takes"              # measured: DESIGN.md "Chains per call"
CAP_BYTES = 1 << 30
CHAIN0 = 11
SEED = 0x1234567812345678
PAD = 64                       # doubles of sentinel band before and after every output


SIGMA_SPIKES = [0.02, 3.1, 3.12, -3.1]   # (theta, phi) of the first and the last vertex of a spike chain: both poles, phi at the cut


def pins(B):
    """the chains compared one by one: both ends, and the three around the edge"""
    return sorted({b for b in (0, 1, 65534, 65535, 65536, B - 1) if 0 <= b < B})


def spike_chains(B):
    return sorted({b for b in (0, 65534, 65535, 65536, B - 1) if 0 <= b < B})


def batch_sizes(case):
    """the batch sizes a case runs at (besides B = 1)"""
    if case.above == "refuses":
        return [B_EDGE]
    return [B_EDGE, B_BIG] if case.rides in ("y", "z", "y/16") else [B_BIG]


Case = collections.namedtuple("Case", "op shape symbols kind rides above split doubles work")


def _id(c):
    return c.op + "".join(f"-{v}" for v in c.shape.values())


def case_bytes(c, B):
    return B * (8 * c.doubles + c.work) + 2 * PAD * 8 * 16


CASES = []


def _add(op, shapes, symbols, kind, rides, split, doubles, work=0, above=None):
    for shape in shapes:
        n = doubles(**shape) if callable(doubles) else doubles
        w = work(**shape) if callable(work) else work
        CASES.append(Case(op, shape, tuple(symbols), kind, rides, above or ("takes" if rides[0] != "y" or Y_ABOVE == "takes" else "refuses"),
                          split, n, w))


KINDS = ("harmonic", "quartic", "rotor")
PATHS = [dict(kind=k, M=M) for k in KINDS for M in (4, 8)]
ROTORS = [dict(M=4), dict(M=8)]
LAT = [dict(kind=k, Mt=m) for k in ("schwinger", "sigma") for m in (2, 4)] + [dict(kind="gff", Mt=4)]
SCHW = [dict(Mt=2), dict(Mt=4)]
SIG = [dict(Mt=2), dict(Mt=4)]
LEVELS = [dict(Mt=m, rotated=r) for m in (2, 4) for r in (0, 1)]
PARTNERED = [l for l in LEVELS if not (l["rotated"] and l["Mt"] == 2)]   # the rotated 2 x 2 level has no coarse partner (1 x 1)
GFFL = [dict(Mt=4, level=0), dict(Mt=8, level=1)]


def lat_n(kind, Mt, **_):
    return (1 if kind == "gff" else 2) * Mt * Mt


def level_n(Mt, rotated=0, **_):
    return 2 * (Mt * Mt // 2 if rotated else Mt * Mt)


# ---- 1-D paths --------------------------------------------------------------------------------------------------------------------
_add("path_evaluate", PATHS, ["mlmcpi_path_evaluate"], "map", "y", 1e-13, lambda kind, M: 2 * M + 8)
_add("path_force", PATHS, ["mlmcpi_path_force"], "map", "y", "bits", lambda kind, M: 6 * M)
_add("path_qoi", [dict(M=4), dict(M=8)], ["mlmcpi_qoi_xsquared", "mlmcpi_qoi_susceptibility"], "map", "y", 1e-13, lambda M: 4 * M + 8)
_add("path_transfers", [dict(M=4), dict(M=8)], ["mlmcpi_path_copy_from_fine", "mlmcpi_path_copy_from_coarse"], "map", "y", "bits",
     lambda M: 12 * M)
_add("path_initialise", PATHS, ["mlmcpi_path_initialise"], "draw", "y", "bits", lambda kind, M: 4 * M)
_add("path_hmc_draw", PATHS, ["mlmcpi_path_hmc_draw", "mlmcpi_path_hmc_workspace_bytes"], "draw", "y", 1e-10, lambda kind, M: 6 * M + 30,
     lambda kind, M: 8 * M + 32 + 8 + 16)
for _M, _rides in ((4, "y"), (64, "x")):   # M = 4: the segmented plan, dim3(nseg, B) and hmc_accept_kernel; M = 64: hmc_chain_kernel
    _add("path_hmc_run", [dict(kind=k, M=_M) for k in KINDS],
         ["mlmcpi_path_hmc_run", "mlmcpi_path_hmc_workspace_bytes", "mlmcpi_path_hmc_run_layout", "mlmcpi_path_hmc_plan"], "draw", _rides, 1e-10,
         lambda kind, M: 6 * M + 30, lambda kind, M: 8 * M + 32 + 8 + 16)
_add("path_site_updates", ROTORS, ["mlmcpi_path_site_updates"], "draw", "x/64", "bits", lambda M: 4 * M)
_add("path_twolevel", PATHS, ["mlmcpi_path_twolevel_draw", "mlmcpi_path_twolevel_draw_masked", "mlmcpi_path_twolevel_workspace_bytes"],
     "draw", "x", 1e-10, lambda kind, M: 16 * M + 60, lambda kind, M: 32 * M + 64)
_add("path_exact_draw", [dict(M=16)], ["mlmcpi_path_exact_draw"], "draw", "y/16", 1e-11, 64)
_add("path_cluster_draw", ROTORS, ["mlmcpi_path_cluster_draw"], "draw", "x/4", "bits", lambda M: 4 * M + 4)
_add("path_correlator", [dict(kind="harmonic", M=4), dict(kind="rotor", M=8)],
     ["mlmcpi_path_correlator", "mlmcpi_path_correlator_workspace_bytes", "mlmcpi_path_correlator_plan"], "map", "linear", "bits",
     lambda kind, M: 4 * M + 40, 256)
_add("path_sweep_draw", ROTORS, ["mlmcpi_path_sweep_draw", "mlmcpi_path_sweep_draw_from", "mlmcpi_path_sweep_draw_qoi"], "draw", "y", "bits",
     lambda M: 12 * M + 30, above="refuses")

# ---- 2-D lattices -----------------------------------------------------------------------------------------------------------------
_add("lattice_evaluate", LAT, ["mlmcpi_lattice_evaluate"], "map", "y", 1e-13, lambda **s: 2 * lat_n(**s) + 8)
_add("lattice_force", LAT, ["mlmcpi_lattice_force"], "map", "y", "bits", lambda **s: 6 * lat_n(**s))
_add("lattice_qoi", LAT, ["mlmcpi_qoi_phi_squared", "mlmcpi_qoi_avg_plaquette", "mlmcpi_qoi_2d_susceptibility",
                          "mlmcpi_qoi_magnetic_susceptibility"], "map", "y", 1e-13, lambda **s: 2 * lat_n(**s) + 16)
_add("lattice_initialise", LAT, ["mlmcpi_lattice_initialise"], "draw", "y", 1e-12, lambda **s: 4 * lat_n(**s), lambda **s: 16 * lat_n(**s))
_add("lattice_sweep_draw", LAT, ["mlmcpi_lattice_sweep_draw", "mlmcpi_lattice_sweep_draw_pingpong", "mlmcpi_lattice_sweep_draw_from",
                                 "mlmcpi_lattice_sweep_plan"], "draw", "y", "bits", lambda **s: 14 * lat_n(**s))
_add("lattice_sweep_draw_qoi", LAT, ["mlmcpi_lattice_sweep_draw_qoi", "mlmcpi_lattice_sweep_draw_qoi_record"], "draw", "y", 1e-13,
     lambda **s: 12 * lat_n(**s) + 60, 64)
_add("lattice_site_updates", LAT, ["mlmcpi_lattice_site_updates"], "draw", "x/64", "bits", lambda **s: 4 * lat_n(**s))
_add("lattice_random_sweep", LAT, ["mlmcpi_lattice_random_sweep_draw", "mlmcpi_lattice_random_sweep_workspace_bytes",
                                   "mlmcpi_lattice_random_sweep_order"], "draw", "x", "bits", lambda **s: 8 * lat_n(**s),
     lambda **s: 64 * lat_n(**s) + 256)
_add("lattice_transfers", [dict(kind="schwinger", Mt=4), dict(kind="gff", Mt=4)],
     ["mlmcpi_lattice_copy_from_fine", "mlmcpi_lattice_copy_from_coarse"], "map", "y", "bits", lambda **s: 12 * lat_n(**s))
_add("lattice_twolevel", [dict(Mt=4, cfa=0), dict(Mt=4, cfa=1)],
     ["mlmcpi_lattice_twolevel_draw", "mlmcpi_lattice_twolevel_draw_cfa", "mlmcpi_lattice_twolevel_workspace_bytes"], "draw", "y", 2e-10,
     lambda Mt, cfa: 16 * Mt * Mt + 30, lambda Mt, cfa: 64 * Mt * Mt + 1024)
_add("lattice_exact_draw", [dict(Mt=4)], ["mlmcpi_lattice_exact_draw", "mlmcpi_lattice_exact_workspace_bytes"], "draw", "y", 1e-12,
     lambda Mt: 4 * Mt * Mt, lambda Mt: 16 * Mt * Mt)
_add("lattice_hmc", [dict(kind="schwinger", Mt=2), dict(kind="schwinger", Mt=4), dict(kind="gff", Mt=4)],
     ["mlmcpi_lattice_hmc_draw", "mlmcpi_lattice_hmc_workspace_bytes"], "draw", "y", 1e-10, lambda **s: 6 * lat_n(**s) + 30,
     lambda **s: 48 * lat_n(**s) + 1024)
_add("wilson_loops", SCHW, ["mlmcpi_schwinger_wilson_loops", "mlmcpi_schwinger_wilson_loops_workspace_bytes",
                            "mlmcpi_schwinger_wilson_loops_plan"], "map", "linear", "bits", lambda Mt: 4 * Mt * Mt + 6 * Mt * Mt, lambda Mt: 8 * Mt * Mt + 256)
_add("schwinger_cluster", SCHW, ["mlmcpi_schwinger_cluster_init", "mlmcpi_schwinger_cluster_draw", "mlmcpi_schwinger_cluster_links",
                                 "mlmcpi_schwinger_cluster_workspace_bytes"], "draw", "x/4", "bits", lambda Mt: 12 * Mt * Mt, 8)
_add("sigma_cluster_draw", SIG, ["mlmcpi_sigma_cluster_draw", "mlmcpi_sigma_cluster_workspace_bytes"], "draw", "x", "bits",
     lambda Mt: 8 * Mt * Mt + 4, lambda Mt: 13 * Mt * Mt + 256)
_add("sigma_sw_draw", SIG, ["mlmcpi_sigma_sw_draw", "mlmcpi_sigma_sw_workspace_bytes"], "draw", "x", "bits", lambda Mt: 8 * Mt * Mt + 12,
     lambda Mt: 21 * Mt * Mt + 256)

# ---- GFF levels -------------------------------------------------------------------------------------------------------------------
_add("gff_level_evaluate", GFFL, ["mlmcpi_gff_level_evaluate", "mlmcpi_gff_cfa_evaluate"], "map", "x", 1e-10, lambda Mt, level: 2 * Mt * Mt + 16)
_add("gff_level_transfers", GFFL, ["mlmcpi_gff_copy_from_fine", "mlmcpi_gff_copy_from_coarse"], "map", "y", "bits", lambda Mt, level: 8 * Mt * Mt)
_add("gff_level_draw", GFFL, ["mlmcpi_gff_level_draw", "mlmcpi_gff_cfa_fill"], "draw", "x", 1e-11, lambda Mt, level: 8 * Mt * Mt + 8)
_add("gff_twolevel", GFFL, ["mlmcpi_gff_twolevel_draw", "mlmcpi_gff_twolevel_workspace_bytes"], "draw", "y", 1e-10,
     lambda Mt, level: 8 * Mt * Mt + 30, lambda Mt, level: 24 * Mt * Mt + 1024)

# ---- sigma-model levels (sigma_levels.hip, sigma_twolevel.hip, sigma_correlator.hip refuse above the edge; their tests pin that) ----
_add("sigma_level_maps", PARTNERED, ["mlmcpi_sigma_level_evaluate", "mlmcpi_sigma_level_magnetic_susceptibility", "mlmcpi_sigma_cfa_evaluate"],
     "map", "y", 1e-13, lambda **s: 2 * level_n(**s) + 24, above="refuses")
_add("sigma_level_draws", PARTNERED, ["mlmcpi_sigma_level_initialise", "mlmcpi_sigma_level_sweep_draw", "mlmcpi_sigma_cfa_fill"], "draw", "y",
     "bits", lambda **s: 12 * level_n(**s), above="refuses")
_add("sigma_level_transfers", PARTNERED, ["mlmcpi_sigma_level_copy_from_fine", "mlmcpi_sigma_level_copy_from_coarse"], "map", "y", "bits",
     lambda **s: 8 * level_n(**s), above="refuses")
_add("sigma_level_correlator", LEVELS, ["mlmcpi_sigma_level_correlator", "mlmcpi_sigma_level_correlator_workspace_bytes"], "map", "z", "bits",
     lambda **s: 2 * level_n(**s) + 8 * (s["Mt"] + 2), lambda **s: 64 * s["Mt"] + 512, above="refuses")
_add("sigma_twolevel", PARTNERED, ["mlmcpi_sigma_twolevel_draw", "mlmcpi_sigma_twolevel_workspace_bytes"], "draw", "y", "bits",
     lambda **s: 8 * level_n(**s) + 30, lambda **s: 24 * level_n(**s) + 1024, above="refuses")
_add("sigma_level_cluster", LEVELS, ["mlmcpi_sigma_level_cluster_draw", "mlmcpi_sigma_level_cluster_workspace_bytes",
                                     "mlmcpi_sigma_level_cluster_improved_draw", "mlmcpi_sigma_level_cluster_improved_workspace_bytes"],
     "draw", "x", "bits", lambda **s: 8 * level_n(**s) + 8 * (s["Mt"] + 8), lambda **s: 40 * level_n(**s) + 512)
_add("sigma_level_sw", LEVELS, ["mlmcpi_sigma_level_sw_draw", "mlmcpi_sigma_level_sw_workspace_bytes", "mlmcpi_sigma_level_sw_structure_draw",
                                "mlmcpi_sigma_level_sw_structure_workspace_bytes", "mlmcpi_sigma_level_sw_correlator_draw",
                                "mlmcpi_sigma_level_sw_correlator_workspace_bytes"], "draw", "x", "bits",
     lambda **s: 12 * level_n(**s) + 8 * (s["Mt"] + 16), lambda **s: 160 * level_n(**s) + 1024)

# ---- statistics -------------------------------------------------------------------------------------------------------------------
_add("stats", [dict(window=3)], ["mlmcpi_stats_accumulate", "mlmcpi_stats_window_record"], "map", "x/256", "bits", 60)

IDS = [_id(c) for c in CASES]

# exports with a `uint32_t B` that no case runs, each with its reason
EXCLUSIONS = {}


# ---- inputs: one row per chain, the same row whatever the batch (a batch of B takes the first B rows) ------------------------------
@functools.lru_cache(maxsize=8)
def uniforms(n, salt=0):
    """[B_BIG, n] uniforms in [0, 1); row b belongs to chain b"""
    u = np.random.default_rng(20261020 + 1000 * n + salt).random((B_BIG, n))
    u.setflags(write=False)
    return u


def path_spikes(kind, M):
    """the spike values of path_cases.path_input on its spike sites; one split here, so the sites are 0 and M - 1"""
    sites = [0, M - 1]
    if kind == "rotor":
        return sites, [2.9 - 0.31 * i if i % 2 else -2.9 + 0.31 * i for i in range(len(sites))]
    return sites, [(6.0 + 0.25 * i) * (-1) ** i for i in range(len(sites))]


@functools.lru_cache(maxsize=4)
def path_input(kind, M):
    """[B_BIG, M]: path_cases.path_input's distributions; the chains at both ends and around the edge carry its spikes.  Rotor
    differences keep 1e-5 away from the branch cut of mod_2pi."""
    u = uniforms(M, salt=KINDS.index(kind))
    sites, values = path_spikes(kind, M)
    if kind == "rotor":
        x = np.pi * (2 * u - 1)
        x[np.array(spike_chains(B_BIG))[:, None], sites] = values
        for _ in range(40):
            d = mod_2pi(x.astype(LD) - np.roll(x, 1, axis=1).astype(LD))
            bad = np.abs(np.abs(d) - PI) < 1e-5
            if not bad.any():
                break
            x[bad] += 0.05
        else:
            raise AssertionError("rotor input still at the branch cut")
    else:
        x = 6 * u - 3
        x[np.array(spike_chains(B_BIG))[:, None], sites] = values
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=4)
def lattice_input(kind, Mt):
    """[B_BIG, n]: Schwinger links in (-pi, pi) with every plaquette 1e-5 away from the branch cut; GFF fields in (-3, 3); sigma
    angles theta in (0.1, pi - 0.1), phi in (-pi, pi).  The spike chains carry +-2.9 (Schwinger), +-6 (GFF) on their first and
    last entry."""
    import lattice_reference as lr
    n = lat_n(kind, Mt)
    u = uniforms(n, salt=7 + ("schwinger", "gff", "sigma").index(kind))
    sp = np.array(spike_chains(B_BIG))[:, None]
    if kind == "gff":
        x = 6 * u - 3
        x[sp, [0, n - 1]] = [6.0, -6.25]
    elif kind == "sigma":
        x = np.empty_like(u)
        x[:, 0::2] = 0.1 + (np.pi - 0.2) * u[:, 0::2]
        x[:, 1::2] = np.pi * (2 * u[:, 1::2] - 1)
        x[sp, [0, 1, n - 2, n - 1]] = SIGMA_SPIKES
    else:
        x = np.pi * (2 * u - 1)
        x[sp, [0, n - 1]] = [2.9, -2.59]
        for _ in range(40):
            P = lr.schwinger_plaquettes(x, Mt, Mt)
            bad = np.abs(np.abs(mod_2pi(P)) - PI) < 1e-5      # [B, vertex]; plaquette v holds the link 2 v
            if not bad.any():
                break
            b, v = np.nonzero(bad)
            x[b, 2 * v] += 0.05
        else:
            raise AssertionError("Schwinger input still at the branch cut")
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=4)
def level_input(Mt, rotated):
    """[B_BIG, 2 n] sigma angles on a level"""
    n2 = level_n(Mt, rotated)
    u = uniforms(n2, salt=31 + rotated)
    x = np.empty_like(u)
    x[:, 0::2] = 0.1 + (np.pi - 0.2) * u[:, 0::2]
    x[:, 1::2] = np.pi * (2 * u[:, 1::2] - 1)
    x[np.array(spike_chains(B_BIG))[:, None], [0, 1, n2 - 2, n2 - 1]] = SIGMA_SPIKES
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=4)
def plain_input(n, salt, scale=1.0):
    """[B_BIG, n] in (-scale, scale) (GFF level fields, statistics samples); the spike chains carry +-6 scale on their first and
    last entry"""
    x = scale * (2 * uniforms(n, salt=salt) - 1)
    x[np.array(spike_chains(B_BIG))[:, None], [0, n - 1]] = [6.0 * scale, -6.25 * scale]
    x.setflags(write=False)
    return x


def window_state(series, window):
    """the state of mlmcpi_stats_window_record after the samples series [n, B], from the definition (common/statistics.cc:4-27), in
    long double: [n, average, S_0 .. S_{W-1}, head, ring[W]] per chain, S_k the average of Q_j Q_{j-k} over j >= k, sample j in
    ring slot (j + 1) mod W, head the slot of the last one.  n >= W, so that every S_k has terms."""
    q = np.asarray(series, dtype=LD)
    n, B = q.shape
    assert n >= window
    out = np.zeros((B, 2 * window + 3), dtype=LD)
    out[:, 0], out[:, 1] = n, q.mean(axis=0)
    for k in range(window):
        out[:, 2 + k] = (q[k:] * q[:n - k]).sum(axis=0) / LD(n - k)
    out[:, 2 + window] = n % window
    for j in range(n - window, n):
        out[:, 3 + window + (j + 1) % window] = q[j]
    return out


class GffLevel:
    """library-side handle of a level of the CoarsenRotate hierarchy of a square GFF lattice (host functions need no GPU)"""
    ROTATE = 4

    def __init__(self, Mt, level, mass, n_gibbs=0, omega=1.0):
        import ctypes as C
        from mlmcpathintegral_amd import abi
        self.abi, self.h = abi, C.c_void_p()
        abi.call("mlmcpi_gff_level_create", Mt, Mt, self.ROTATE, level, float(mass), n_gibbs, float(omega), C.byref(self.h))
        n, nc, mtc, mxc, mu2 = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_double()
        abi.call("mlmcpi_gff_level_info", self.h, C.byref(n), C.byref(nc), C.byref(mtc), C.byref(mxc), C.byref(mu2))
        self.N, self.n_coarse, self.Mt_c, self.mu2 = n.value, nc.value, mtc.value, mu2.value
        self.Mt, self.level, self.mass, self.n_gibbs, self.omega, self.rotated = Mt, level, mass, n_gibbs, omega, level % 2 == 1

    def nb(self):
        import ctypes as C
        out = np.zeros(8 * self.N, dtype=np.uint32)
        self.abi.call("mlmcpi_neighbours_2d", self.Mt, self.Mt, int(self.rotated), out.ctypes.data_as(C.c_void_p))
        return out.reshape(self.N, 8)

    def tables(self):
        import ctypes as C
        pairs, fineonly = np.zeros(2 * self.n_coarse, dtype=np.uint32), np.zeros(self.N - self.n_coarse, dtype=np.uint32)
        self.abi.call("mlmcpi_gff_level_tables", self.h, pairs.ctypes.data_as(C.c_void_p), fineonly.ctypes.data_as(C.c_void_p))
        return pairs, fineonly

    def matrix(self, which):
        import ctypes as C
        out = np.zeros((self.N, self.N))
        self.abi.call("mlmcpi_gff_level_matrix", self.h, which, out.ctypes.data_as(C.c_void_p))
        return out

    def oracle(self):
        """the oracle's handle of the same level"""
        import oracle
        L = oracle.lib()
        return L, L.orc_gff_level_new(self.Mt, self.Mt, self.ROTATE, self.level, float(self.mass), self.n_gibbs, float(self.omega))


def lattice_transfers_oracle(kind, Mt, lo, B, tall=True):
    """the outputs of the lattice_transfers runner from the oracle's copies: on ONE lattice of B Mt columns (chain-major storage is
    the chains stacked along j, and a copy reads within blocks of rx columns), or chain by chain"""
    import oracle
    L = oracle.lib()
    n = lat_n(kind, Mt)
    fine = lattice_input(kind, Mt)[lo:lo + B]
    out = {}
    for rt, rx in ((2, 2), (2, 1), (1, 2)):
        nc = n // (rt * rx)
        new_coarse = np.ascontiguousarray(0.5 * fine[:, :nc])
        groups = [(np.ascontiguousarray(fine).reshape(-1), new_coarse.reshape(-1), B)] if tall else \
                 [(np.ascontiguousarray(fine[b]), new_coarse[b], 1) for b in range(B)]
        coarse, back = [], []
        for f, c_new, nb in groups:
            c, f2 = np.zeros(nb * nc), f.copy()
            if kind == "schwinger":
                L.orc_schwinger_copy_from_fine(Mt // rt, nb * Mt // rx, rt, rx, f, c)
                L.orc_schwinger_copy_from_coarse(Mt // rt, nb * Mt // rx, rt, rx, np.ascontiguousarray(c_new), f2)
            else:
                L.orc_gff_transfer(Mt // rt, nb * Mt // rx, rt, rx, f.copy(), c, 1)
                L.orc_gff_transfer(Mt // rt, nb * Mt // rx, rt, rx, f2, np.ascontiguousarray(c_new).copy(), 0)
            coarse.append(c.reshape(nb, nc))
            back.append(f2.reshape(nb, n))
        out[f"coarse{rt}{rx}"], out[f"fine{rt}{rx}"] = np.concatenate(coarse), np.concatenate(back)
    return out
