"""CPU: the gradient-flow model of tests/sigma_flow_reference.py -- the order of the scheme (and that the test can tell it from
the second-order variant), the invariants of the definition (the energy never rises, a planar spin wave is a fixed point, the
instanton and dislocation tables, step lists), and the input conditions of every GPU comparison.  The records of one run are in
profiles/sigma_flow.json (written into the directory MLMCPI_SIGMA_FLOW_RECORDS names, if set)."""
import numpy as np
import pytest

import sigma_cooling_reference as cool
import sigma_flow_reference as ref
import sigma_topology_reference as topo

LD = np.longdouble
_id = lambda k: "%dx%d-%s-%d" % (k[0], k[1], "rot" if k[2] else "plain", k[3])   # noqa: E731


def _field_at(rot, eps, project_stages=False, t=0.5):
    phi = topo.uniform_spins(8, 8, rot, 1, seed=2024)
    return ref.flow(8, 8, rot, phi, eps, [int(round(t / eps))], with_float64=False, project_stages=project_stages).sig


@pytest.fixture(scope="module")
def fine():
    return {rot: _field_at(rot, 1.0 / 1024) for rot in (False, True)}


def _ratios(rot, fine, project_stages):
    err = [float(np.abs(_field_at(rot, 1.0 / d, project_stages) - fine[rot]).max()) for d in (16, 32, 64)]
    return err[0] / err[1], err[1] / err[2]


@pytest.mark.parametrize("rot", [False, True])
def test_the_scheme_is_third_order(fine, rot):
    """the error at t = 0.5 against eps = 1/1024 falls by about 8 on halving eps: 1/16 -> 1/32 and 1/32 -> 1/64, 8 x 8"""
    r = _ratios(rot, fine, False)
    print(f"{'rotated' if rot else 'plain'}: error ratios {r[0]:.3f}, {r[1]:.3f}")
    ref.record("sigma_flow.json", "order_%s" % ("rotated" if rot else "plain"), list(r))
    assert all(6.0 <= x <= 10.0 for x in r), r


@pytest.mark.parametrize("rot", [False, True])
def test_projecting_every_stage_is_second_order(fine, rot):
    """the control: the same run with every stage normalised falls by about 4, so the test above tells the two apart"""
    r = _ratios(rot, fine, True)
    print(f"{'rotated' if rot else 'plain'}, stages projected: error ratios {r[0]:.3f}, {r[1]:.3f}")
    ref.record("sigma_flow.json", "order_stage_projection_%s" % ("rotated" if rot else "plain"), list(r))
    assert all(3.0 <= x <= 5.0 for x in r), r


@pytest.mark.parametrize("eps", [0.05, 0.1, 0.25])
@pytest.mark.parametrize("rot", [False, True])
def test_energy_never_rises(rot, eps):
    """200 steps from uniform random spins; the allowance is the rounding of a sum of 2 n terms <= 2 in the model's arithmetic"""
    phi = topo.uniform_spins(8, 8, rot, 4, seed=77)
    c = ref.flow(8, 8, rot, phi, eps, list(range(201)), with_float64=False)
    allowance = 4 * c.n * 2 * topo.EPS_LONGDOUBLE
    assert np.all(np.diff(c.E, axis=1) <= allowance), float(np.diff(c.E, axis=1).max())
    assert np.all(c.E >= -allowance) and np.all(c.E[:, -1] < c.E[:, 0])


@pytest.mark.parametrize("Mt,Mx,m", [(8, 8, 1), (18, 10, 1), (18, 10, 2)])
@pytest.mark.parametrize("rot", [False, True])
def test_a_planar_spin_wave_is_a_fixed_point(Mt, Mx, rot, m):
    """theta_l = pi / 2, phi_l = 2 pi m i / Mt: Delta_l = c sigma_l, c = 2 + 2 cos k (plain) or 4 cos k (rotated), k = 2 pi m / Mt, so
    F = 0.  The float64 angles are within d0 = 2^-51 + 2^-53 of the wave (half an ulp of a phase below 2 pi, cos(fl(pi / 2))).  Around
    the wave in-plane deviations obey a discrete heat equation with weights cos k > 0 and 1 (they do not grow), out-of-plane ones
    z' = Lap z + (4 - c) z (they grow at most as exp((4 - c) t)); a step adds rounding of at most (256 eps + 8) u (three forces of
    <= 21 operations on values <= 4 weighted by b_i sum <= 2, the normalisation).  So after s steps, t = s eps,
        |sigma^s - sigma^0| <= 2 [d0 (1 + exp((4 - c) t)) + s (256 eps + 8) u exp((4 - c) t)]
    the factor 2 for the discrete scheme against the continuous growth."""
    eps, s = 0.05, 20
    n = cool.n_vertices(Mt, Mx, rot)
    i, _ = cool.coords(Mt, Mx, rot)
    k = 2 * np.pi * m / Mt
    phi = np.empty((1, 2 * n))
    phi[0, 0::2], phi[0, 1::2] = np.pi / 2, k * i
    c = 4 * np.cos(k) if rot else 2 + 2 * np.cos(k)
    assert np.cos(k) > 0
    f = ref.flow(Mt, Mx, rot, phi, eps, [0, s], with_float64=False)
    grow = np.exp((4 - c) * s * eps)
    bound = 2 * ((2.0 ** -51 + 2.0 ** -53) * (1 + grow) + s * (256 * eps + 8) * topo.EPS_LONGDOUBLE * grow)
    drift = float(np.abs(f.sig - cool.sigma_of(phi, n, LD)).max())
    print(f"({Mt}, {Mx}) {'rotated' if rot else 'plain'} m = {m}: drift {drift:.3e}, bound {bound:.3e}")
    assert drift <= bound
    assert np.abs(f.E[0, 1] - f.E[0, 0]) <= 4 * n * bound and np.all(np.abs(f.Q) < 1e-12)


@pytest.mark.parametrize("k", [1, 2])
def test_instantons_on_the_plain_level_keep_their_charge(k):
    Q, E = ref.instanton_table(16, 16, False, 3.0, k, tuple(ref.INSTANTON_STEPS))
    assert np.all(np.rint(Q) == k), Q
    assert np.all(np.diff(E) <= 1e-12) and E[-1] >= k * 0.5


@pytest.mark.parametrize("rot", [False, True])
def test_the_dislocation_loses_its_charge(rot):
    """the model measures the step count from which round(Q) = 0; ref.DISLOCATION_LOSS_STEP fixes it (t = 0.5 plain, 0.25 rotated)"""
    DISLOCATION_LOSS_STEP = ref.DISLOCATION_LOSS_STEP
    Q, E = ref.instanton_table(*ref.DISLOCATION[:2], rot, *ref.DISLOCATION[2:], tuple(ref.DISLOCATION_STEPS))
    s = ref.DISLOCATION_STEPS[ref.charge_loss_step(Q)]
    print(f"dislocation, {'rotated' if rot else 'plain'}: round(Q) = 0 from step {s} (t = {s * ref.TABLE_EPS:.2f}); E_0 / 4 pi = {E[0]:.6f}")
    ref.record("sigma_flow.json", "dislocation_loss_%s" % ("rotated" if rot else "plain"),
               {"eps": ref.TABLE_EPS, "step": s, "t": s * ref.TABLE_EPS, "Q": Q.tolist()})
    assert np.rint(Q[0]) == 1 and s == DISLOCATION_LOSS_STEP[rot], (s, Q)
    assert np.all(np.diff(E) <= 1e-12)


def test_every_gpu_case_has_a_seed():
    assert set(ref.SEEDS) == set(ref.gpu_cases())


@pytest.mark.parametrize("key", ref.gpu_cases(), ids=_id)
def test_input_conditions(key):
    """min |Y| >= 0.5 at every normalisation and charge margin >= 1e-6 at every listed step count, for every GPU comparison input
    and both of its runs"""
    _, runs = ref.gpu_case(*key)
    assert len(runs) == len(ref.case_runs(key))
    for c in runs:
        print(f"{_id(key)} eps = {c.eps}: min |Y| = {c.min_norm:.3g}, margin = {c.margin.min():.3g}, dev64 = {c.dev64.max():.3g}")
        assert c.min_norm >= ref.MIN_NORM
        assert c.margin.min() >= ref.MIN_MARGIN
        # float64 stays with longdouble closely enough that the bounds built on it can still tell one charge from the next
        assert c.q_bound().max() < 0.01 and c.e_bound().max() < 1e-6 * c.n


@pytest.mark.parametrize("rot", [False, True])
def test_step_lists(rot):
    """Q_s, E_s and the field from [s] are those from any list containing s"""
    phi = topo.uniform_spins(6, 4, rot, 5, seed=99)
    full = ref.flow(6, 4, rot, phi, 0.05, [0, 1, 2, 5])
    for k, s in enumerate(full.depths):
        one = ref.flow(6, 4, rot, phi, 0.05, [s])
        assert np.array_equal(one.Q[:, 0], full.Q[:, k]) and np.array_equal(one.E[:, 0], full.E[:, k])
    assert np.array_equal(ref.flow(6, 4, rot, phi, 0.05, [5]).sig, full.sig)
    assert np.array_equal(ref.flow(6, 4, rot, phi, 0.05, [2, 5]).Q[:, 1], full.Q[:, 3])


def test_step_zero_is_the_charge_reference():
    phi = topo.uniform_spins(6, 4, True, 5, seed=7)
    c0, c = topo.charge(6, 4, True, phi), ref.flow(6, 4, True, phi, 0.05, [0])
    assert np.array_equal(c0.Q, c.Q[:, 0]) and np.array_equal(c0.margin, c.margin[:, 0])
    c1 = cool.cool(6, 4, True, phi, [0])
    assert np.array_equal(c1.E, c.E)


def test_flow_scale_interpolates_and_refuses_what_is_not_bracketed():
    t, y = [0.0, 0.5, 1.0, 2.0], [0.0, 0.02, 0.05, 0.07]
    assert ref.flow_scale(t, y, 0.035) == pytest.approx(0.75)
    assert ref.flow_scale(t, y, 0.05) == pytest.approx(1.0)
    assert np.isnan(ref.flow_scale(t, y, 0.1)) and np.isnan(ref.flow_scale(t, y, -0.01)) and np.isnan(ref.flow_scale([1.0], [0.05], 0.05))
