"""Thin torch-tensor front end of the C ABI, used by tests and bench.py.

PyTorch is plumbing only: it owns device memory and the stream; every computation goes through
libmlmcpi_hip.so.  All state tensors are float64 CUDA tensors of shape [B, n] in the reference's
SampleState layout (see include/mlmcpi_hip.h).
"""
import ctypes as C

import torch

from . import abi
from .abi import GFF, HARMONIC, NONLINEAR_SIGMA, QUARTIC, ROTOR, SCHWINGER  # noqa: F401


def _p(t):
    if t is None:
        return C.c_void_p(0)
    assert t.is_cuda and t.is_contiguous(), "device, contiguous tensors only"
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f64(B, n, like):
    return torch.empty((B, n), dtype=torch.float64, device=like.device)


def _check_state(x, n):
    assert x.dtype == torch.float64 and x.dim() == 2 and x.shape[1] == n, (x.shape, n)


def _workspace(query, *args, device="cuda"):
    """uint8 tensor of the size the ABI's `query`(*args, &bytes) asks for"""
    nbytes = C.c_size_t(0)
    abi.call(query, *args, C.byref(nbytes))
    return torch.empty(nbytes.value, dtype=torch.uint8, device=device)


# ---- 1-D paths -----------------------------------------------------------------------------------
def path_evaluate(act, x):
    _check_state(x, act.M)
    out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
    abi.call("mlmcpi_path_evaluate", C.byref(act), _p(x), x.shape[0], _p(out), _stream())
    return out


def path_force(act, x):
    _check_state(x, act.M)
    f = torch.empty_like(x)
    abi.call("mlmcpi_path_force", C.byref(act), _p(x), _p(f), x.shape[0], _stream())
    return f


def path_initialise(act, B, seed, chain0=0, device="cuda"):
    x = torch.empty((B, act.M), dtype=torch.float64, device=device)
    abi.call("mlmcpi_path_initialise", C.byref(act), _p(x), B, seed, chain0, _stream())
    return x


def qoi_xsquared(x):
    out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
    abi.call("mlmcpi_qoi_xsquared", _p(x), x.shape[1], x.shape[0], _p(out), _stream())
    return out


def qoi_susceptibility(x, T_final):
    out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
    abi.call("mlmcpi_qoi_susceptibility", _p(x), x.shape[1], float(T_final), x.shape[0], _p(out), _stream())
    return out


class PathHMC:
    """HMCSampler::draw on B device-resident chains (sampler/hmcsampler.cc:8-69)."""

    def __init__(self, act, B, nt, dt, n_rep=1, seed=1, chain0=0, device="cuda"):
        self.act, self.B, self.nt, self.dt, self.n_rep, self.seed, self.chain0 = act, B, nt, dt, n_rep, seed, chain0
        self.work = _workspace("mlmcpi_path_hmc_workspace_bytes", C.byref(act), B, nt, device=device)
        self.accept = torch.zeros(B, dtype=torch.int32, device=device)
        self.energies = torch.zeros((B, 4), dtype=torch.float64, device=device)
        self.traj = 0
        self.n_total = 0
        self.n_accepted = torch.zeros(B, dtype=torch.int64, device=device)

    def draw(self, x, count_stats=True):
        _check_state(x, self.act.M)
        abi.call("mlmcpi_path_hmc_draw", C.byref(self.act), _p(x), self.B, self.nt, float(self.dt), self.n_rep,
                 self.seed, self.chain0, self.traj, _p(self.work), _p(self.accept), _p(self.energies), _stream())
        self.traj += self.n_rep
        if count_stats:
            self.n_total += 1
            self.n_accepted += self.accept
        return self.accept


def hmc_thermalise(hmc, x, n, dt_jitter=0.3):
    """Untimed burn-in of B chains from the reference's cold (x = 0) or random start.  A state with no potential
    energy in its stiff modes has a systematic leapfrog energy error ~ M dt^2 <omega^2> / 8 (measured: +2.65 at
    dt = 0.004, +44 at dt = 0.02 for the quartic action, M_lat = 32768, a = 1/32), so a cold chain rejects every
    trajectory at the production step size and stays cold for ever: ramp the step size up from dt / 20, then jitter
    it so that no mode sits at a leapfrog resonance.  The production dt is restored at the end."""
    dt0 = hmc.dt
    ramp = [0.05] * 6 + [0.1] * 6 + [0.2] * 6 + [0.5] * 6
    for k in range(n):
        hmc.dt = dt0 * (ramp[k] if k < len(ramp) else 1.0 + dt_jitter * (((k * 7) % 11) - 5) / 5.0)
        hmc.draw(x, count_stats=False)
    hmc.dt = dt0


def path_hmc_run(hmc, x, n_draws, qoi_kind):
    """n_draws x (HMCSampler::draw + QoI) on the device; returns (q [B, n_draws], accepted draws per chain)."""
    q = torch.empty((hmc.B, n_draws), dtype=torch.float64, device=x.device)
    cnt = torch.zeros(hmc.B, dtype=torch.int32, device=x.device)
    abi.call("mlmcpi_path_hmc_run", C.byref(hmc.act), _p(x), hmc.B, hmc.nt, float(hmc.dt), hmc.n_rep, n_draws, qoi_kind,
             hmc.seed, hmc.chain0, hmc.traj, _p(hmc.work), _p(q), _p(cnt), _stream())
    hmc.traj += n_draws * hmc.n_rep
    if not path_hmc_plan(hmc.act, hmc.B, hmc.nt)["chain_major"]:
        q = q.reshape(n_draws, hmc.B).t().contiguous()
    return q, cnt


def path_hmc_plan(act, B, nt):
    """The launch geometry of PathHMC / path_hmc_run for these arguments (mlmcpi_path_hmc_plan; no device needed): a dict of
    R, NT, nseg, owned_len, halo, chain_major"""
    info = abi.PathHmcPlan()
    abi.call("mlmcpi_path_hmc_plan", C.byref(act), B, nt, C.byref(info))
    return {n: getattr(info, n) for n, _ in abi.PathHmcPlan._fields_}


def path_correlator_plan(act, n_lag, B):
    """The launch geometry of path_correlator for these arguments (mlmcpi_path_correlator_plan; no device needed): a dict of
    the fields of mlmcpi_path_correlator_plan_info"""
    info = abi.PathCorrelatorPlan()
    abi.call("mlmcpi_path_correlator_plan", C.byref(act), n_lag, B, C.byref(info))
    return {n: getattr(info, n) for n, _ in abi.PathCorrelatorPlan._fields_}


def path_correlator_workspace(act, n_lag, B, device="cuda"):
    """workspace of path_correlator for B chains and n_lag lags (uint8 tensor)"""
    return _workspace("mlmcpi_path_correlator_workspace_bytes", C.byref(act), n_lag, B, device=device)


def path_correlator(act, x, n_lag, acc=None, work=None):
    """C(tau), tau = 0 .. n_lag - 1, of every chain of x [B, M] (mlmcpi_path_correlator): returns [B, n_lag]; acc [B, n_lag, 2]
    (optional) is added to: C and C^2"""
    _check_state(x, act.M)
    B = x.shape[0]
    if work is None:
        work = path_correlator_workspace(act, n_lag, B, x.device)
    if acc is not None:
        assert acc.dtype == torch.float64 and tuple(acc.shape) == (B, n_lag, 2), acc.shape
    out = _f64(B, n_lag, x)
    abi.call("mlmcpi_path_correlator", C.byref(act), _p(x), B, n_lag, _p(out), _p(acc), _p(work), work.numel(), _stream())
    return out


class PathTwoLevelStep:
    """TwoLevelMetropolisStep (montecarlo/twolevelmetropolisstep.cc) on B device chains: Gaussian fill-in."""

    def __init__(self, fine, coarse, B, seed=1, chain0=0, device="cuda"):
        self.fine, self.coarse, self.B, self.seed, self.chain0 = fine, coarse, B, seed, chain0
        self.work = _workspace("mlmcpi_path_twolevel_workspace_bytes", C.byref(fine), B, device=device)
        self.accept = torch.zeros(B, dtype=torch.int32, device=device)
        self.terms = torch.zeros((B, 3), dtype=torch.float64, device=device)
        self.theta = torch.zeros((B, fine.M), dtype=torch.float64, device=device)  # current fine state
        self.step = 0

    def set_state(self, x):
        self.theta.copy_(x)

    def draw(self, x_coarse, mask=None):
        """mask (int32 [B], optional): chains with mask == 0 are left alone and come back rejected
        (HierarchicalSampler::draw's `if (not accept) break`, sampler/hierarchicalsampler.cc:62-76)"""
        _check_state(x_coarse, self.coarse.M)
        abi.call("mlmcpi_path_twolevel_draw_masked", C.byref(self.fine), C.byref(self.coarse), _p(x_coarse), _p(self.theta),
                 self.B, self.seed, self.chain0, self.step, _p(self.work), _p(mask) if mask is not None else None,
                 _p(self.accept), _p(self.terms), _stream())
        self.step += 1
        return self.accept


class HOExactSampler:
    """HarmonicOscillatorAction::draw (the exact Gaussian sampler) on B device chains: x = L y on the fp64 matrix
    cores; the Cholesky factor is built once on the host (mlmcpi_ho_cholesky_factor)."""

    def __init__(self, act, B, seed=1, chain0=0, device="cuda"):
        import numpy as np
        self.act, self.B, self.seed, self.chain0 = act, B, seed, chain0
        lt = np.zeros((act.M, act.M))
        abi.call("mlmcpi_ho_cholesky_factor", C.byref(act), lt.ctypes.data_as(C.c_void_p))
        self.LT_host = lt
        self.LT = torch.from_numpy(lt).to(device)
        self.step = 0

    def draw(self, x=None):
        if x is None:
            x = torch.empty((self.B, self.act.M), dtype=torch.float64, device=self.LT.device)
        _check_state(x, self.act.M)
        abi.call("mlmcpi_path_exact_draw", C.byref(self.act), _p(self.LT), _p(x), self.B, self.seed, self.chain0, self.step,
                 _stream())
        self.step += 1
        return x


class GFFExactSampler:
    """GFFAction::draw (exact Gaussian sampler) on B device chains by spectral synthesis (batched 2-D FFT)."""

    def __init__(self, act, B, seed=1, chain0=0, device="cuda"):
        self.act, self.B, self.seed, self.chain0 = act, B, seed, chain0
        self.work = _workspace("mlmcpi_lattice_exact_workspace_bytes", C.byref(act), B, device=device)
        self.step = 0

    def draw(self, phi=None):
        if phi is None:
            phi = torch.empty((self.B, self.act.Mt * self.act.Mx), dtype=torch.float64, device=self.work.device)
        _check_state(phi, self.act.Mt * self.act.Mx)
        abi.call("mlmcpi_lattice_exact_draw", C.byref(self.act), _p(phi), self.B, self.seed, self.chain0, self.step,
                 _p(self.work), _stream())
        self.step += 1
        return phi


class LatticeTwoLevelStep:
    """TwoLevelMetropolisStep on the Schwinger lattice, semi-coarsening (ExpCos fill-in), B device chains."""

    def __init__(self, fine, coarse, B, seed=1, chain0=0, device="cuda", cfa_kind=0):
        """cfa_kind 0: the conditioned fine action the reference's factory picks for the lattice; 1: the Gaussian variant
        (QuenchedSchwingerGaussianConditionedFineAction; lattices coarsened in both directions)"""
        self.fine, self.coarse, self.B, self.seed, self.chain0, self.cfa_kind = fine, coarse, B, seed, chain0, cfa_kind
        self.work = _workspace("mlmcpi_lattice_twolevel_workspace_bytes", C.byref(fine), C.byref(coarse), B, device=device)
        self.accept = torch.zeros(B, dtype=torch.int32, device=device)
        self.terms = torch.zeros((B, 3), dtype=torch.float64, device=device)
        self.theta = torch.zeros((B, 2 * fine.Mt * fine.Mx), dtype=torch.float64, device=device)  # current fine state
        self.step = 0

    def set_state(self, x):
        self.theta.copy_(x)

    def draw(self, phi_coarse):
        _check_state(phi_coarse, 2 * self.coarse.Mt * self.coarse.Mx)
        abi.call("mlmcpi_lattice_twolevel_draw_cfa", C.byref(self.fine), C.byref(self.coarse), self.cfa_kind, _p(phi_coarse),
                 _p(self.theta), self.B, self.seed, self.chain0, self.step, _p(self.work), _p(self.accept), _p(self.terms),
                 _stream())
        self.step += 1
        return self.accept


def path_sweep_draw(act, x, scratch, n_overrelax, n_heatbath, seed, chain0, sweep0):
    _check_state(x, act.M)
    abi.call("mlmcpi_path_sweep_draw", C.byref(act), _p(x), _p(scratch), x.shape[0], n_overrelax, n_heatbath, seed,
             chain0, sweep0, _stream())


def path_sweep_draw_qoi(act, src, w0, w1, n_overrelax, n_heatbath, seed, chain0, sweep0, acc=None):
    """draw + topological susceptibility in one pass (mlmcpi_path_sweep_draw_qoi; rotor): reads `src` (w1 may be src),
    returns (result tensor, the other work tensor, chi [B]); acc [B, 5]: record_sample of chi in the same call."""
    _check_state(src, act.M)
    where = C.c_int32(0)
    q = torch.empty(src.shape[0], dtype=torch.float64, device=src.device)
    if acc is not None:
        assert acc.shape == (src.shape[0], 5) and acc.dtype == torch.float64 and acc.is_contiguous()
    abi.call("mlmcpi_path_sweep_draw_qoi", C.byref(act), _p(src), _p(w0), _p(w1), src.shape[0], n_overrelax, n_heatbath, seed,
             chain0, sweep0, _p(q), None if acc is None else _p(acc), C.byref(where), _stream())
    return (w0, w1, q) if where.value == 0 else (w1, w0, q)


def _site_args(x, sites):
    """(d_sites, n, single) for the site-update entry points: an int, or a uint32 / int32 device tensor of site indices"""
    if isinstance(sites, int):
        return None, 1, sites
    assert sites.is_cuda and sites.dtype in (torch.int32, torch.uint32) and sites.is_contiguous()
    return C.c_void_p(sites.data_ptr()), sites.numel(), 0


def path_site_updates(act, x, sites, heat, seed, chain0, step):
    """Action::heatbath_update / overrelaxation_update(state, l) (rotor): the sites in order, all chains of x in place"""
    _check_state(x, act.M)
    d, n, single = _site_args(x, sites)
    abi.call("mlmcpi_path_site_updates", C.byref(act), _p(x), x.shape[0], d, n, single, int(bool(heat)), seed, chain0, step, _stream())


def lattice_site_updates(act, x, sites, heat, seed, chain0, step):
    _check_state(x, lattice_size(act))
    d, n, single = _site_args(x, sites)
    abi.call("mlmcpi_lattice_site_updates", C.byref(act), _p(x), x.shape[0], d, n, single, int(bool(heat)), seed, chain0, step, _stream())


def path_cluster_draw(act, x, n_updates, seed, chain0, update0, count=True):
    """ClusterSampler::draw on a 1-D lattice (rotor): n_updates reflection-cluster updates of every chain of x, in place;
    returns the flipped sites per chain of this call (int32 [B]; None with count=False)"""
    _check_state(x, act.M)
    sites = torch.zeros(x.shape[0], dtype=torch.int32, device=x.device) if count else None
    abi.call("mlmcpi_path_cluster_draw", C.byref(act), _p(x), x.shape[0], n_updates, seed, chain0, update0, _p(sites), _stream())
    return sites


class SchwingerClusterSampler:
    """QuenchedSchwingerClusterSampler on B device chains: the state is the plaquette path psi [B, Mt Mx]."""

    def __init__(self, act, B, n_updates=10, seed=1, chain0=0, device="cuda"):
        self.act, self.B, self.n_updates, self.seed, self.chain0 = act, B, n_updates, seed, chain0
        nbytes = C.c_size_t(0)
        abi.call("mlmcpi_schwinger_cluster_workspace_bytes", C.byref(act), B, C.byref(nbytes))
        self.work = torch.zeros(nbytes.value // 4, dtype=torch.int32, device=device)
        self.psi = torch.empty((B, act.Mt * act.Mx), dtype=torch.float64, device=device)
        abi.call("mlmcpi_schwinger_cluster_init", C.byref(act), _p(self.psi), B, seed, chain0, _stream())
        self.draws = 0

    def draw(self, theta):
        _check_state(theta, 2 * self.act.Mt * self.act.Mx)
        abi.call("mlmcpi_schwinger_cluster_draw", C.byref(self.act), _p(self.psi), _p(theta), self.B, self.n_updates, self.seed,
                 self.chain0, self.draws, _p(self.work), _stream())
        self.draws += 1

    def cluster_sites(self):
        return self.work[:self.B]


def schwinger_cluster_links(act, psi, gauge, seed, chain0, draw0):
    """the link field of a plaquette path (mlmcpi_schwinger_cluster_links): theta [B, 2 Mt Mx]"""
    _check_state(psi, act.Mt * act.Mx)
    theta = torch.empty((psi.shape[0], 2 * act.Mt * act.Mx), dtype=torch.float64, device=psi.device)
    abi.call("mlmcpi_schwinger_cluster_links", C.byref(act), _p(psi), _p(theta), psi.shape[0], int(gauge), seed, chain0, draw0,
             _stream())
    return theta


# ---- 2-D lattices ---------------------------------------------------------------------------------
def lattice_size(act):
    n = C.c_uint32(0)
    abi.call("mlmcpi_lattice_state_size", C.byref(act), C.byref(n))
    return n.value


def lattice_evaluate(act, phi):
    out = torch.empty(phi.shape[0], dtype=torch.float64, device=phi.device)
    abi.call("mlmcpi_lattice_evaluate", C.byref(act), _p(phi), phi.shape[0], _p(out), _stream())
    return out


def lattice_force(act, phi):
    f = torch.empty_like(phi)
    abi.call("mlmcpi_lattice_force", C.byref(act), _p(phi), _p(f), phi.shape[0], _stream())
    return f


def lattice_initialise(act, B, seed, chain0=0, device="cuda"):
    phi = torch.empty((B, lattice_size(act)), dtype=torch.float64, device=device)
    abi.call("mlmcpi_lattice_initialise", C.byref(act), _p(phi), B, seed, chain0, _stream())
    return phi


def lattice_sweep_draw(act, phi, scratch, n_overrelax, n_heatbath, seed, chain0, sweep0, fuse=0):
    _check_state(phi, lattice_size(act))
    abi.call("mlmcpi_lattice_sweep_draw", C.byref(act), _p(phi), _p(scratch), phi.shape[0], n_overrelax, n_heatbath,
             seed, chain0, sweep0, fuse, _stream())


# enum mlmcpi_sweep_kernel -> the instantiation a record names, as a demangler prints it
_SWEEP_KERNELS = [
    lambda l: "schwinger_sweep_kernel<%s, %d, %d, %d, %s>" % (_b(l["n_heatbath"]), l["threads"], l["tile_w"] * l["fixed_tile"],
                                                               l["tile_h"] * l["fixed_tile"], _b(l["step"])),
    lambda l: "gff_sweep_kernel<%s, %d, %d, %d>" % (_b(l["n_heatbath"]), l["threads"], l["tile_w"] * l["fixed_tile"],
                                                     l["tile_h"] * l["fixed_tile"]),
    lambda l: "schwinger_or_block_kernel<%d>" % l["n_overrelax"],
    lambda l: "gff_or_block_kernel<%d, %d>" % (l["n_overrelax"], l["tile_w"]),
    lambda l: "gff_or_heat_kernel<%d, %d>" % (l["n_overrelax"], l["tile_w"]),
    lambda l: "schwinger_perm_kernel<%d>" % l["tile_h"],
    lambda l: "schwinger_perm_heat_kernel<%d, %s>" % (l["threads"], _b(l["step"])),
    lambda l: "sigma_sweep_kernel<%d>" % l["threads"],
]


def _b(v):
    return "true" if v else "false"


def lattice_sweep_plan(act, B, n_overrelax, n_heatbath, fuse=0):
    """The launches of lattice_sweep_draw* for these arguments under the options in force (mlmcpi_lattice_sweep_plan; no
    device needed): one dict per launch with the fields of mlmcpi_sweep_launch and "instantiation", the kernel it names."""
    count, capacity = C.c_uint32(0), max(1, n_overrelax + n_heatbath)   # a launch covers at least one sweep
    recs = (abi.SweepLaunch * capacity)()
    abi.call("mlmcpi_lattice_sweep_plan", C.byref(act), B, n_overrelax, n_heatbath, fuse, recs, capacity, C.byref(count))
    plan = [{n: getattr(r, n) for n, _ in abi.SweepLaunch._fields_} for r in recs[:count.value]]
    for l in plan:
        l["instantiation"] = _SWEEP_KERNELS[l["kernel"]](l)
    return plan


def lattice_random_sweep_workspace(act, B, device="cuda"):
    """workspace of lattice_random_sweep_draw for B chains (uint8 tensor)"""
    return _workspace("mlmcpi_lattice_random_sweep_workspace_bytes", C.byref(act), B, device=device)


def lattice_random_sweep_draw(act, phi, n_overrelax, n_heatbath, seed, chain0, sweep0, work=None):
    """OverrelaxedHeatBathSampler::draw with random_order = true, parallel within a chain (mlmcpi_lattice_random_sweep_draw):
    n_overrelax + n_heatbath sweeps of phi, in place, every sweep in its own random order (Philox purpose 18)"""
    _check_state(phi, lattice_size(act))
    if work is None:
        work = lattice_random_sweep_workspace(act, phi.shape[0], phi.device)
    abi.call("mlmcpi_lattice_random_sweep_draw", C.byref(act), _p(phi), phi.shape[0], n_overrelax, n_heatbath, seed, chain0, sweep0,
             _p(work), _stream())


def sigma_cluster_workspace(act, B, device="cuda"):
    """workspace of sigma_cluster_draw for B chains (uint8 tensor)"""
    return _workspace("mlmcpi_sigma_cluster_workspace_bytes", C.byref(act), B, device=device)


def sigma_cluster_draw(act, x, n_updates, seed, chain0, update0, count=True, work=None):
    """Wolff single-cluster updates of the O(3) sigma model (mlmcpi_sigma_cluster_draw): n_updates updates of every chain of
    x [B, 2 Mt Mx], in place, update counters update0 + k; returns the flipped sites per chain of this call (int32 [B]; None
    with count=False)"""
    _check_state(x, lattice_size(act))
    if work is None:
        work = sigma_cluster_workspace(act, x.shape[0], x.device)
    sites = torch.zeros(x.shape[0], dtype=torch.int32, device=x.device) if count else None
    abi.call("mlmcpi_sigma_cluster_draw", C.byref(act), _p(x), x.shape[0], n_updates, seed, chain0, update0, _p(sites), _p(work),
             _stream())
    return sites


def sigma_sw_workspace(act, B, device="cuda"):
    """workspace of sigma_sw_draw for B chains (uint8 tensor)"""
    return _workspace("mlmcpi_sigma_sw_workspace_bytes", C.byref(act), B, device=device)


def sigma_sw_draw(act, x, n_updates, seed, chain0, update0, outputs=True, work=None):
    """Swendsen-Wang multi-cluster updates of the O(3) sigma model (mlmcpi_sigma_sw_draw): n_updates updates of every chain of
    x [B, 2 Mt Mx], in place, update counters update0 + k; returns, per chain and summed over this call's updates, (flipped
    vertices int32 [B], clusters int32 [B], improved chi_m float64 [B]), or None with outputs=False"""
    _check_state(x, lattice_size(act))
    B = x.shape[0]
    if work is None:
        work = sigma_sw_workspace(act, B, x.device)
    flipped = clusters = improved = None
    if outputs:
        flipped = torch.zeros(B, dtype=torch.int32, device=x.device)
        clusters = torch.zeros(B, dtype=torch.int32, device=x.device)
        improved = torch.zeros(B, dtype=torch.float64, device=x.device)
    abi.call("mlmcpi_sigma_sw_draw", C.byref(act), _p(x), B, n_updates, seed, chain0, update0, _p(flipped), _p(clusters), _p(improved),
             _p(work), _stream())
    return (flipped, clusters, improved) if outputs else None


# ---- O(3) sigma model: levels of the CoarsenRotate hierarchy and the two-level step ---------------------------------
def sigma_level_size(level):
    n = C.c_uint32(0)
    abi.call("mlmcpi_sigma_level_state_size", C.byref(level), C.byref(n))
    return n.value


def sigma_level_initialise(level, B, seed, chain0=0, device="cuda"):
    x = torch.empty((B, sigma_level_size(level)), dtype=torch.float64, device=device)
    abi.call("mlmcpi_sigma_level_initialise", C.byref(level), _p(x), B, seed, chain0, _stream())
    return x


def sigma_level_evaluate(level, x):
    _check_state(x, sigma_level_size(level))
    out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
    abi.call("mlmcpi_sigma_level_evaluate", C.byref(level), _p(x), x.shape[0], _p(out), _stream())
    return out


def sigma_level_magnetic_susceptibility(level, x):
    _check_state(x, sigma_level_size(level))
    out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
    abi.call("mlmcpi_sigma_level_magnetic_susceptibility", C.byref(level), _p(x), x.shape[0], _p(out), _stream())
    return out


def sigma_level_topological_charge(level, x, acc=None):
    """geometric topological charge of every chain of x [B, 2 n] on a level, rotated or not (mlmcpi_sigma_level_topological_charge):
    returns (Q [B], chi = Q^2 / n [B]); acc [B, 5] (optional): record_sample of chi in the same call"""
    _check_state(x, sigma_level_size(level))
    B = x.shape[0]
    if acc is not None:
        assert acc.dtype == torch.float64 and tuple(acc.shape) == (B, 5), acc.shape
    q = torch.empty(B, dtype=torch.float64, device=x.device)
    chi = torch.empty(B, dtype=torch.float64, device=x.device)
    abi.call("mlmcpi_sigma_level_topological_charge", C.byref(level), _p(x), B, _p(q), _p(chi), _p(acc), _stream())
    return q, chi


def sigma_level_cooling_workspace(level, B, device="cuda"):
    """workspace of sigma_level_cooled_charge for B chains (uint8 tensor)"""
    return _workspace("mlmcpi_sigma_level_cooling_workspace_bytes", C.byref(level), B, device=device)


def sigma_level_cooling_plan(level, B, depths):
    """the launches mlmcpi_sigma_level_cooled_charge would make (abi.SigmaCoolingPlan; host only)"""
    d = (C.c_uint32 * len(depths))(*depths)
    plan = abi.SigmaCoolingPlan()
    abi.call("mlmcpi_sigma_level_cooling_plan", C.byref(level), B, d, len(depths), C.byref(plan))
    return plan


def _sigma_level_smoothed_charge(name, workspace, level, x, lead, counts, energy, field, stream, work):
    """what sigma_level_cooled_charge and sigma_level_flowed_charge share; lead: the arguments between B and the list (eps)"""
    _check_state(x, sigma_level_size(level))
    B, nd = x.shape[0], len(counts)
    d = (C.c_uint32 * nd)(*counts)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        if work is None:
            work = workspace(level, B, x.device)
        q, chi = _f64(B, nd, x), _f64(B, nd, x)
        e = _f64(B, nd, x) if energy else None
        out = torch.empty_like(x) if field else None
        abi.call(name, C.byref(level), _p(x), B, *lead, d, nd, _p(q), _p(chi), _p(e), _p(out), _p(work), work.numel(), _stream())
    return (q, chi) + ((e,) if energy else ()) + ((out,) if field else ())


def sigma_level_cooled_charge(level, x, depths, *, energy=False, cooled=False, stream=None, work=None):
    """cooling of every chain of x [B, 2 n] on a level, rotated or not, measured at the ascending list `depths` of sweep counts
    (mlmcpi_sigma_level_cooled_charge; x is not written): returns (Q [B, n_depths], chi = Q^2 / n [B, n_depths]), then with
    energy=True the bond energy E [B, n_depths] and with cooled=True the angles [B, 2 n] of the field at the last depth.  Runs,
    and allocates, on `stream` (a torch.cuda.Stream; default: the current one)."""
    return _sigma_level_smoothed_charge("mlmcpi_sigma_level_cooled_charge", sigma_level_cooling_workspace, level, x, (), depths, energy,
                                        cooled, stream, work)


def sigma_level_flow_workspace(level, B, device="cuda"):
    """workspace of sigma_level_flowed_charge for B chains (uint8 tensor)"""
    return _workspace("mlmcpi_sigma_level_flow_workspace_bytes", C.byref(level), B, device=device)


def sigma_level_flow_plan(level, B, eps, steps):
    """the launches mlmcpi_sigma_level_flowed_charge would make (abi.SigmaFlowPlan; host only)"""
    d = (C.c_uint32 * len(steps))(*steps)
    plan = abi.SigmaFlowPlan()
    abi.call("mlmcpi_sigma_level_flow_plan", C.byref(level), B, eps, d, len(steps), C.byref(plan))
    return plan


def sigma_level_flowed_charge(level, x, eps, steps, *, energy=False, flowed=False, stream=None, work=None):
    """gradient flow of every chain of x [B, 2 n] on a level, rotated or not, in steps of size eps (0 < eps <= 0.25), measured at
    the ascending list `steps` of step counts, flow time t = s eps (mlmcpi_sigma_level_flowed_charge; x is not written): returns
    (Q [B, n_steps], chi = Q^2 / n [B, n_steps]), then with energy=True the bond energy E [B, n_steps] and with flowed=True the
    angles [B, 2 n] of the field at the last step count.  Runs, and allocates, on `stream` (a torch.cuda.Stream; default: the
    current one)."""
    return _sigma_level_smoothed_charge("mlmcpi_sigma_level_flowed_charge", sigma_level_flow_workspace, level, x, (eps,), steps, energy,
                                        flowed, stream, work)


def sigma_level_correlator_size(level):
    """n_out = (Mt/2 + 1) + (Mx/2 + 1): the lags of C_t, then those of C_x"""
    n = C.c_uint32(0)
    abi.call("mlmcpi_sigma_level_correlator_size", C.byref(level), C.byref(n))
    return n.value


def sigma_level_correlator_workspace(level, B, device="cuda"):
    """workspace of sigma_level_correlator for B chains (uint8 tensor)"""
    return _workspace("mlmcpi_sigma_level_correlator_workspace_bytes", C.byref(level), B, device=device)


def sigma_level_correlator(level, x, acc=None, work=None):
    """time-slice correlators of every chain of x [B, 2 n] on a level, rotated or not (mlmcpi_sigma_level_correlator): returns
    [B, n_out], C_t(0 .. Mt/2) then C_x(0 .. Mx/2); acc [B, n_out, 2] (optional) is added to: C and C^2"""
    _check_state(x, sigma_level_size(level))
    B, n_out = x.shape[0], sigma_level_correlator_size(level)
    if work is None:
        work = sigma_level_correlator_workspace(level, B, x.device)
    if acc is not None:
        assert acc.dtype == torch.float64 and tuple(acc.shape) == (B, n_out, 2), acc.shape
    out = _f64(B, n_out, x)
    abi.call("mlmcpi_sigma_level_correlator", C.byref(level), _p(x), B, _p(out), _p(acc), _p(work), work.numel(), _stream())
    return out


def sigma_level_sweep_draw(level, x, scratch, n_overrelax, n_heatbath, seed, chain0, sweep0):
    """OverrelaxedHeatBathSampler::draw on a level, in place"""
    _check_state(x, sigma_level_size(level))
    assert scratch.shape == x.shape and scratch.dtype == x.dtype
    abi.call("mlmcpi_sigma_level_sweep_draw", C.byref(level), _p(x), _p(scratch), x.shape[0], n_overrelax, n_heatbath, seed, chain0,
             sweep0, _stream())
    return x


def sigma_level_copy_from_fine(fine_level, fine):
    _check_state(fine, sigma_level_size(fine_level))
    coarse = _f64(fine.shape[0], sigma_level_size(fine_level) // 2, fine)   # half of the vertices are coarse
    abi.call("mlmcpi_sigma_level_copy_from_fine", C.byref(fine_level), _p(fine), _p(coarse), fine.shape[0], _stream())
    return coarse


def sigma_level_copy_from_coarse(fine_level, coarse, fine):
    _check_state(fine, sigma_level_size(fine_level))
    _check_state(coarse, sigma_level_size(fine_level) // 2)
    abi.call("mlmcpi_sigma_level_copy_from_coarse", C.byref(fine_level), _p(coarse), _p(fine), fine.shape[0], _stream())
    return fine


def sigma_level_cluster_workspace(level, B, device="cuda"):
    """workspace of sigma_level_cluster_draw for B chains (uint8 tensor)"""
    return _workspace("mlmcpi_sigma_level_cluster_workspace_bytes", C.byref(level), B, device=device)


def sigma_level_cluster_draw(level, x, n_updates, seed, chain0, update0, count=True, work=None):
    """Wolff single-cluster updates on a level, rotated or not (mlmcpi_sigma_level_cluster_draw): n_updates updates of every
    chain of x [B, 2 n], in place, update counters update0 + k; returns the flipped vertices per chain of this call (int32 [B];
    None with count=False)"""
    _check_state(x, sigma_level_size(level))
    if work is None:
        work = sigma_level_cluster_workspace(level, x.shape[0], x.device)
    sites = torch.zeros(x.shape[0], dtype=torch.int32, device=x.device) if count else None
    abi.call("mlmcpi_sigma_level_cluster_draw", C.byref(level), _p(x), x.shape[0], n_updates, seed, chain0, update0, _p(sites),
             _p(work), _stream())
    return sites


def sigma_level_cluster_improved_workspace(level, B, device="cuda"):
    """workspace of sigma_level_cluster_improved_draw for B chains (uint8 tensor): the plain draw's plus the slice table"""
    return _workspace("mlmcpi_sigma_level_cluster_improved_workspace_bytes", C.byref(level), B, device=device)


def sigma_level_cluster_improved_draw(level, x, n_updates, seed, chain0, update0, work=None, structure=False, correlator=False):
    """sigma_level_cluster_draw with the improved estimators of the single cluster (mlmcpi_sigma_level_cluster_improved_draw): the
    same state; returns, per chain and summed over this call's updates, (flipped vertices int32 [B], improved chi_m float64 [B]),
    then with structure=True the improved structure factors (F_t, F_x) float64 [B, 2], then with correlator=True the improved
    time-slice correlators float64 [B, n_out] in the layout of sigma_level_correlator"""
    _check_state(x, sigma_level_size(level))
    B = x.shape[0]
    if work is None:
        work = sigma_level_cluster_improved_workspace(level, B, x.device)
    sites = torch.zeros(B, dtype=torch.int32, device=x.device)
    improved = torch.zeros(B, dtype=torch.float64, device=x.device)
    factors = torch.zeros(B, 2, dtype=torch.float64, device=x.device) if structure else None
    corr = torch.zeros(B, sigma_level_correlator_size(level), dtype=torch.float64, device=x.device) if correlator else None
    abi.call("mlmcpi_sigma_level_cluster_improved_draw", C.byref(level), _p(x), B, n_updates, seed, chain0, update0, _p(sites),
             _p(improved), _p(factors), _p(corr), _p(work), work.numel(), _stream())
    return (sites, improved) + ((factors,) if structure else ()) + ((corr,) if correlator else ())


def sigma_level_sw_workspace(level, B, device="cuda"):
    """workspace of sigma_level_sw_draw for B chains (uint8 tensor)"""
    return _workspace("mlmcpi_sigma_level_sw_workspace_bytes", C.byref(level), B, device=device)


def sigma_level_sw_structure_workspace(level, B, device="cuda"):
    """workspace of sigma_level_sw_draw(..., structure=True) for B chains (uint8 tensor): 32 B per vertex and chain more"""
    return _workspace("mlmcpi_sigma_level_sw_structure_workspace_bytes", C.byref(level), B, device=device)


def sigma_level_sw_correlator_workspace(level, B, device="cuda"):
    """workspace of sigma_level_sw_draw(..., correlator=True) for B chains (uint8 tensor): the plain draw's plus the slice tables"""
    return _workspace("mlmcpi_sigma_level_sw_correlator_workspace_bytes", C.byref(level), B, device=device)


def sigma_level_sw_draw(level, x, n_updates, seed, chain0, update0, outputs=True, work=None, structure=False, correlator=False):
    """Swendsen-Wang multi-cluster updates on a level, rotated or not (mlmcpi_sigma_level_sw_draw): n_updates updates of every
    chain of x [B, 2 n], in place, update counters update0 + k; returns, per chain and summed over this call's updates, (flipped
    vertices int32 [B], clusters int32 [B], improved chi_m float64 [B]), or None with outputs=False.  structure=True
    (mlmcpi_sigma_level_sw_structure_draw; `work` from sigma_level_sw_structure_workspace): the same state and outputs and a fourth
    tensor, float64 [B, 2], the improved structure factors (F_t, F_x) at the lowest momentum summed over this call's updates.
    correlator=True (mlmcpi_sigma_level_sw_correlator_draw; `work` from sigma_level_sw_correlator_workspace; exclusive with
    structure=True): the same state and outputs and a fourth tensor, float64 [B, n_out] in the layout of sigma_level_correlator,
    the cluster-improved time-slice correlators C_t then C_x summed over this call's updates"""
    _check_state(x, sigma_level_size(level))
    B = x.shape[0]
    if structure and correlator:
        raise ValueError("structure=True and correlator=True are exclusive: F and xi_2 follow from the improved correlator")
    if work is None:
        work = (sigma_level_sw_correlator_workspace if correlator else
                sigma_level_sw_structure_workspace if structure else sigma_level_sw_workspace)(level, B, x.device)
    flipped = clusters = improved = None
    if outputs:
        flipped = torch.zeros(B, dtype=torch.int32, device=x.device)
        clusters = torch.zeros(B, dtype=torch.int32, device=x.device)
        improved = torch.zeros(B, dtype=torch.float64, device=x.device)
    if structure:
        if not outputs:
            raise ValueError("structure=True returns outputs")
        factors = torch.zeros(B, 2, dtype=torch.float64, device=x.device)
        abi.call("mlmcpi_sigma_level_sw_structure_draw", C.byref(level), _p(x), B, n_updates, seed, chain0, update0, _p(flipped),
                 _p(clusters), _p(improved), _p(factors), _p(work), work.numel(), _stream())
        return flipped, clusters, improved, factors
    if correlator:
        if not outputs:
            raise ValueError("correlator=True returns outputs")
        corr = torch.zeros(B, sigma_level_correlator_size(level), dtype=torch.float64, device=x.device)
        abi.call("mlmcpi_sigma_level_sw_correlator_draw", C.byref(level), _p(x), B, n_updates, seed, chain0, update0, _p(flipped),
                 _p(clusters), _p(improved), _p(corr), _p(work), work.numel(), _stream())
        return flipped, clusters, improved, corr
    abi.call("mlmcpi_sigma_level_sw_draw", C.byref(level), _p(x), B, n_updates, seed, chain0, update0, _p(flipped), _p(clusters),
             _p(improved), _p(work), _stream())
    return (flipped, clusters, improved) if outputs else None


def sigma_cfa_fill(fine_level, x, seed, chain0, step):
    """NonlinearSigmaConditionedFineAction::fill_fine_points, in place"""
    _check_state(x, sigma_level_size(fine_level))
    abi.call("mlmcpi_sigma_cfa_fill", C.byref(fine_level), _p(x), x.shape[0], seed, chain0, step, _stream())
    return x


def sigma_cfa_evaluate(fine_level, x):
    _check_state(x, sigma_level_size(fine_level))
    out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
    abi.call("mlmcpi_sigma_cfa_evaluate", C.byref(fine_level), _p(x), x.shape[0], _p(out), _stream())
    return out


class SigmaTwoLevelStep:
    """TwoLevelMetropolisStep between a sigma-model level and its CoarsenRotate partner, B device chains."""

    def __init__(self, fine, coarse, B, seed=1, chain0=0, device="cuda"):
        self.fine, self.coarse, self.B, self.seed, self.chain0 = fine, coarse, B, seed, chain0
        self.work = _workspace("mlmcpi_sigma_twolevel_workspace_bytes", C.byref(fine), B, device=device)
        self.accept = torch.zeros(B, dtype=torch.int32, device=device)
        self.terms = torch.zeros((B, 3), dtype=torch.float64, device=device)
        self.theta = torch.zeros((B, sigma_level_size(fine)), dtype=torch.float64, device=device)  # current fine state
        self.step = 0

    def set_state(self, x):
        self.theta.copy_(x)

    def trial(self):
        """the trial state of the last draw (a view of the workspace)"""
        return self.work[:self.theta.numel() * 8].view(torch.float64).view(self.theta.shape)

    def draw(self, phi_coarse):
        _check_state(phi_coarse, sigma_level_size(self.coarse))
        abi.call("mlmcpi_sigma_twolevel_draw", C.byref(self.fine), C.byref(self.coarse), _p(phi_coarse), _p(self.theta), self.B,
                 self.seed, self.chain0, self.step, _p(self.work), _p(self.accept), _p(self.terms), _stream())
        self.step += 1
        return self.accept


def lattice_random_sweep_order(act, B, seed, chain0, sweep, rounds=True, device="cuda"):
    """the visiting order (int32 [B, n]) and the round of every index (int32 [B, n], or None) of that sweep"""
    n = (2 if act.kind == abi.SCHWINGER else 1) * act.Mt * act.Mx
    order = torch.empty((B, n), dtype=torch.int32, device=device)
    rnd = torch.empty((B, n), dtype=torch.int32, device=device) if rounds else None
    abi.call("mlmcpi_lattice_random_sweep_order", C.byref(act), B, seed, chain0, sweep, _p(order), _p(rnd), _stream())
    return order, rnd


def lattice_sweep_draw_pingpong(act, a, b, n_overrelax, n_heatbath, seed, chain0, sweep0, fuse=0):
    """Sweeps without the final copy; returns (state, scratch) -- the tensors swapped when needed."""
    _check_state(a, lattice_size(act))
    flag = C.c_int32(0)
    abi.call("mlmcpi_lattice_sweep_draw_pingpong", C.byref(act), _p(a), _p(b), a.shape[0], n_overrelax, n_heatbath,
             seed, chain0, sweep0, fuse, C.byref(flag), _stream())
    return (b, a) if flag.value else (a, b)


def lattice_sweep_draw_qoi(act, src, w0, w1, n_overrelax, n_heatbath, seed, chain0, sweep0, qoi_kind, fuse=0, acc=None):
    """draw + QoI in one pass (mlmcpi_lattice_sweep_draw_qoi): reads `src` (w1 may be src), returns (result tensor, the
    other work tensor, qoi [B]); qoi_kind 1 = average plaquette, 2 = Q^2 / (4 pi^2), 3 = phi^2 (GFF), 4 = chi_m (sigma model).  acc [B, 5]: record_sample of the QoI
    as well, in the same call (mlmcpi_lattice_sweep_draw_qoi_record)."""
    where = C.c_int32(0)
    q = torch.empty(src.shape[0], dtype=torch.float64, device=src.device)
    if acc is None:
        abi.call("mlmcpi_lattice_sweep_draw_qoi", C.byref(act), _p(src), _p(w0), _p(w1), src.shape[0], n_overrelax, n_heatbath, seed,
                 chain0, sweep0, fuse, qoi_kind, _p(q), C.byref(where), _stream())
    else:
        assert acc.shape == (src.shape[0], 5) and acc.dtype == torch.float64 and acc.is_contiguous()
        abi.call("mlmcpi_lattice_sweep_draw_qoi_record", C.byref(act), _p(src), _p(w0), _p(w1), src.shape[0], n_overrelax, n_heatbath,
                 seed, chain0, sweep0, fuse, qoi_kind, _p(q), _p(acc), C.byref(where), _stream())
    return (w0, w1, q) if where.value == 0 else (w1, w0, q)


def lattice_copy_from_fine(fine_act, rt, rx, fine):
    """Action::copy_from_fine on the device; returns the coarse-level state [B, n_coarse]."""
    n = lattice_size(fine_act) // (rt * rx)
    coarse = torch.empty((fine.shape[0], n), dtype=torch.float64, device=fine.device)
    abi.call("mlmcpi_lattice_copy_from_fine", C.byref(fine_act), rt, rx, _p(fine), _p(coarse), fine.shape[0], _stream())
    return coarse


def lattice_copy_from_coarse(fine_act, rt, rx, coarse, fine):
    """Action::copy_from_coarse on the device: updates the coarse-level entries of `fine` in place."""
    abi.call("mlmcpi_lattice_copy_from_coarse", C.byref(fine_act), rt, rx, _p(coarse), _p(fine), fine.shape[0], _stream())


def path_copy_from_fine(fine):
    coarse = torch.empty((fine.shape[0], fine.shape[1] // 2), dtype=torch.float64, device=fine.device)
    abi.call("mlmcpi_path_copy_from_fine", _p(fine), _p(coarse), coarse.shape[1], fine.shape[0], _stream())
    return coarse


def path_copy_from_coarse(coarse, fine):
    abi.call("mlmcpi_path_copy_from_coarse", _p(coarse), _p(fine), coarse.shape[1], fine.shape[0], _stream())


def qoi_phi_squared(phi):
    out = torch.empty(phi.shape[0], dtype=torch.float64, device=phi.device)
    abi.call("mlmcpi_qoi_phi_squared", _p(phi), phi.shape[1], phi.shape[0], _p(out), _stream())
    return out


def qoi_avg_plaquette(theta, Mt, Mx):
    out = torch.empty(theta.shape[0], dtype=torch.float64, device=theta.device)
    abi.call("mlmcpi_qoi_avg_plaquette", _p(theta), Mt, Mx, theta.shape[0], _p(out), _stream())
    return out


def wilson_loops_plan(Mt, Mx, R, S, B):
    """The launch geometry of wilson_loops for these arguments (mlmcpi_schwinger_wilson_loops_plan; no device needed): a dict
    of the fields of mlmcpi_wilson_loops_plan_info"""
    info = abi.WilsonLoopsPlan()
    abi.call("mlmcpi_schwinger_wilson_loops_plan", Mt, Mx, R, S, B, C.byref(info))
    return {n: getattr(info, n) for n, _ in abi.WilsonLoopsPlan._fields_}


def wilson_loops_workspace(Mt, Mx, R, S, B, device="cuda"):
    """workspace of wilson_loops for B chains and loops up to R x S (uint8 tensor)"""
    return _workspace("mlmcpi_schwinger_wilson_loops_workspace_bytes", Mt, Mx, R, S, B, device=device)


def wilson_loops(theta, Mt, Mx, R, S, acc=None, work=None):
    """W(r, s), r <= R, s <= S, of every chain of theta [B, 2 Mt Mx] (mlmcpi_schwinger_wilson_loops): returns [B, R, S], entry
    [r - 1, s - 1]; acc [B, R, S, 2] (optional) is added to: W and W^2"""
    _check_state(theta, 2 * Mt * Mx)
    B = theta.shape[0]
    if work is None:
        work = wilson_loops_workspace(Mt, Mx, R, S, B, theta.device)
    if acc is not None:
        assert acc.dtype == torch.float64 and tuple(acc.shape) == (B, R, S, 2), acc.shape
    out = torch.empty((B, R, S), dtype=torch.float64, device=theta.device)
    abi.call("mlmcpi_schwinger_wilson_loops", _p(theta), Mt, Mx, B, R, S, _p(out), _p(acc), _p(work), work.numel(), _stream())
    return out


def gff_correlator_size(Mt, Mx, n_mom, rotated=False):
    """n_out = n_mom (Mt/2 + 1) + n_mom (Mx/2 + 1) (mlmcpi_gff_correlator_size; no device needed)"""
    n = C.c_uint32(0)
    abi.call("mlmcpi_gff_correlator_size", Mt, Mx, int(bool(rotated)), n_mom, C.byref(n))
    return n.value


def gff_correlator_plan(Mt, Mx, n_mom, rotated=False, n_chains=1):
    """The launch geometry of gff_correlator for these arguments (mlmcpi_gff_correlator_plan; no device needed): a dict of the
    fields of mlmcpi_gff_correlator_plan_info"""
    info = abi.GffCorrelatorPlan()
    abi.call("mlmcpi_gff_correlator_plan", Mt, Mx, int(bool(rotated)), n_mom, n_chains, C.byref(info))
    return {n: getattr(info, n) for n, _ in abi.GffCorrelatorPlan._fields_}


def gff_correlator_workspace(Mt, Mx, n_mom, n_chains, rotated=False, device="cuda"):
    """workspace of gff_correlator for n_chains chains and n_mom momenta (uint8 tensor)"""
    return _workspace("mlmcpi_gff_correlator_workspace_bytes", Mt, Mx, int(bool(rotated)), n_mom, n_chains, device=device)


def gff_correlator(phi, Mt, Mx, n_mom, rotated=False, acc=None, work=None):
    """C_t(tau; q) and C_x(tau; q), q < n_mom, of every chain of the GFF state phi [B, N] on the level (Mt, Mx, rotated)
    (mlmcpi_gff_correlator): returns [B, n_out], C_t first, momentum-major, lag fastest (gff_correlator_t / _x slice it); acc
    [B, n_out, 2] (optional) is added to: C and C^2"""
    _check_state(phi, Mt * Mx // 2 if rotated else Mt * Mx)
    B, n_out = phi.shape[0], gff_correlator_size(Mt, Mx, n_mom, rotated)
    if work is None:
        work = gff_correlator_workspace(Mt, Mx, n_mom, B, rotated, phi.device)
    if acc is not None:
        assert acc.dtype == torch.float64 and tuple(acc.shape) == (B, n_out, 2), acc.shape
    out = torch.empty((B, n_out), dtype=torch.float64, device=phi.device)
    abi.call("mlmcpi_gff_correlator", Mt, Mx, int(bool(rotated)), n_mom, _p(phi), B, _p(out), _p(acc), _p(work), work.numel(), _stream())
    return out


def gff_correlator_t(out, Mt, Mx, n_mom, q):
    """C_t(tau; q), tau = 0 .. Mt/2, of every chain: the view [B, Mt/2 + 1] of what gff_correlator returned"""
    assert 0 <= q < n_mom and out.shape[-1] == n_mom * (Mt // 2 + Mx // 2 + 2)
    nt = Mt // 2 + 1
    return out[..., q * nt:(q + 1) * nt]


def gff_correlator_x(out, Mt, Mx, n_mom, q):
    """C_x(tau; q), tau = 0 .. Mx/2, of every chain: the view [B, Mx/2 + 1] of what gff_correlator returned"""
    assert 0 <= q < n_mom and out.shape[-1] == n_mom * (Mt // 2 + Mx // 2 + 2)
    nt, nx = Mt // 2 + 1, Mx // 2 + 1
    return out[..., n_mom * nt + q * nx:n_mom * nt + (q + 1) * nx]


def qoi_2d_susceptibility(theta, Mt, Mx):
    out = torch.empty(theta.shape[0], dtype=torch.float64, device=theta.device)
    abi.call("mlmcpi_qoi_2d_susceptibility", _p(theta), Mt, Mx, theta.shape[0], _p(out), _stream())
    return out


def qoi_magnetic_susceptibility(phi, Mt, Mx):
    """QoI2DMagneticSusceptibility of sigma-model states [B, 2 Mt Mx]: |sum_n sigma_n|^2 / (Mt Mx) per chain"""
    _check_state(phi, 2 * Mt * Mx)
    out = torch.empty(phi.shape[0], dtype=torch.float64, device=phi.device)
    abi.call("mlmcpi_qoi_magnetic_susceptibility", _p(phi), Mt, Mx, phi.shape[0], _p(out), _stream())
    return out


class LatticeHMC:
    """HMCSampler::draw for a 2-D action (streaming leapfrog)."""

    def __init__(self, act, B, nt, dt, n_rep=1, seed=1, chain0=0, device="cuda"):
        self.act, self.B, self.nt, self.dt, self.n_rep, self.seed, self.chain0 = act, B, nt, dt, n_rep, seed, chain0
        self.work = _workspace("mlmcpi_lattice_hmc_workspace_bytes", C.byref(act), B, device=device)
        self.accept = torch.zeros(B, dtype=torch.int32, device=device)
        self.energies = torch.zeros((B, 4), dtype=torch.float64, device=device)
        self.traj = 0

    def draw(self, phi):
        abi.call("mlmcpi_lattice_hmc_draw", C.byref(self.act), _p(phi), self.B, self.nt, float(self.dt), self.n_rep,
                 self.seed, self.chain0, self.traj, _p(self.work), _p(self.accept), _p(self.energies), _stream())
        self.traj += self.n_rep
        return self.accept


def stats_accumulate(acc, q):
    abi.call("mlmcpi_stats_accumulate", _p(acc), _p(q), q.shape[0], _stream())


def stats_window_state(B, window, device="cuda"):
    """zeroed state of mlmcpi_stats_window_record for B chains"""
    return torch.zeros((B, 2 * window + 3), dtype=torch.float64, device=device)


def stats_window_record(state, q):
    """Statistics::record_sample with the autocorrelation window, one chain per row of `state`"""
    window = (state.shape[1] - 3) // 2
    abi.call("mlmcpi_stats_window_record", _p(state), _p(q), q.shape[0], window, _stream())


def stats_window_tau_int(state, pooled=True):
    """Statistics::tau_int (common/statistics.cc:38-61) from the windowed state: per chain, or -- pooled -- with the
    autocovariances averaged over the chains of the batch first (one number for the batch)."""
    W = (state.shape[1] - 3) // 2
    n = state[:, 0:1]
    a1 = state[:, 1:2]
    cov = state[:, 2:2 + W] - a1 * a1                                  # [B, W]
    k = torch.arange(W, dtype=torch.float64, device=state.device)[None, :]
    wgt = 1.0 - k / torch.clamp(n, min=1.0)   # (the reference sums ALL k < window, also those the series has not reached: statistics.cc:86-88)
    if pooled:   # a 0-dim device tensor: no synchronisation here (the multilevel driver reads it one sample later)
        c = (cov * wgt).mean(dim=0)
        tau = 1.0 + 2.0 * c[1:].sum() / c[0]
        return torch.clamp(torch.nan_to_num(tau, nan=1.0, posinf=1.0, neginf=1.0), min=1.0)
    tau = 1.0 + 2.0 * (cov * wgt)[:, 1:].sum(dim=1) / cov[:, 0]
    return torch.clamp(torch.nan_to_num(tau, nan=1.0), min=1.0)


# ---- test hooks -------------------------------------------------------------------------------------
def test_random(seed, chain, step, purpose, sub, n, device="cuda"):
    out = torch.empty((n, 4), dtype=torch.float64, device=device)
    abi.call("mlmcpi_test_random", seed, chain, step, purpose, sub, n, _p(out), _stream())
    return out


def test_expcos(seed, chain, step, beta, xp, xm):
    out = torch.empty_like(xp)
    abi.call("mlmcpi_test_expcos", seed, chain, step, float(beta), _p(xp), _p(xm), xp.numel(), _p(out), _stream())
    return out


def test_vs_draw(seed, chain, step, scale, xp, xm):
    out = torch.empty_like(xp)
    abi.call("mlmcpi_test_vs_draw", seed, chain, step, float(scale), _p(xp), _p(xm), xp.numel(), _p(out), _stream())
    return out


def test_math(fn, a, b=None):
    """(out0, out1) = fn(a, b) element by element: one of the fp64 device primitives (abi.MATH_FN: name or number; enum
    mlmcpi_math_fn in include/mlmcpi_hip.h says what each reads and returns).  a, b: float64 device tensors of one size."""
    fn = abi.MATH_FN[fn] if isinstance(fn, str) else int(fn)
    assert a.dtype == torch.float64 and (b is None or (b.dtype == torch.float64 and b.numel() == a.numel()))
    out0, out1 = torch.empty_like(a), torch.empty_like(a)
    abi.call("mlmcpi_test_math", fn, _p(a), _p(b), a.numel(), _p(out0), _p(out1), _stream())
    return out0, out1


def test_expsin2(seed, chain, step, sigma):
    out = torch.empty_like(sigma)
    abi.call("mlmcpi_test_expsin2", seed, chain, step, _p(sigma), sigma.numel(), _p(out), _stream())
    return out
