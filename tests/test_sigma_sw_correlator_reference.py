"""CPU: the cluster-improved time-slice correlator of the Swendsen-Wang update as tests/sigma_sw_correlator_reference.py states
it: the definition by brute force, the two identities against the improved chi_m and structure factor, the mean over the coins
by enumeration, the lag lemma on the model's clusters, the slice table against a dict, the device's integers inside
device_bound, and the law (improved = plain) on a model chain."""
import math
import random

import numpy as np
import pytest

import sigma_correlator_reference as cref
import sigma_level_model as slm
import sigma_level_sw_model as slsw
import sigma_sw_correlator_reference as scr
import sigma_sw_structure_reference as ssr
from conftest import zcheck

LD = np.longdouble
LEVELS = [(2, 2), (2, 6), (6, 2), (4, 4), (16, 16), (66, 34)]


def _cold(L):
    """every spin along one direction"""
    phi = np.empty(2 * L.n)
    phi[0::2], phi[1::2] = 0.5 * math.pi, 0.25
    return phi


def _update(L, seed, regime):
    """a model update in one of three regimes: `mixed` (heat-bath start at L.beta), `singletons` (a random start: few bonds),
    `spanning` (a cold start: at large beta one cluster takes nearly everything)"""
    if regime == "spanning":                             # the first seed whose normal is not nearly orthogonal to the spins
        for s in range(seed, seed + 50):
            info = slsw.dev_update(L, _cold(L), s, 0, 0)[1]
            if np.bincount(info["labels"]).max() > L.n // 2:
                return info
        raise AssertionError("no spanning cluster")
    elif regime == "singletons":
        phi = slm.initialise(L, 1, seed)[0]
    else:
        phi = slm.sweep_draw(L, slm.initialise(L, 1, seed), 10, 1, seed)[0]
    return slsw.dev_update(L, phi, seed, 0, 0)[1]


REGIMES = [("singletons", 0.05), ("mixed", 1.5), ("spanning", 8.0)]


@pytest.mark.parametrize("regime,beta", REGIMES)
@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("Mt,Mx", [(2, 2), (2, 6), (6, 2), (4, 4), (6, 8)])
def test_the_reference_is_the_definition(Mt, Mx, rot, regime, beta):
    L = slm.Level(Mt, Mx, rot, beta)
    info = _update(L, 3 + Mt, regime)
    got, want = scr.improved(L, info["a"], info["labels"]), scr.brute_force(L, info["a"], info["labels"])
    assert got.shape == (cref.n_out(Mt, Mx),)
    assert np.all(np.abs(got - want) <= 1e-17 * L.n)


@pytest.mark.parametrize("regime,beta", REGIMES)
@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("Mt,Mx", LEVELS)
def test_the_weighted_sums_are_the_improved_susceptibility_and_structure_factor(Mt, Mx, rot, regime, beta):
    """sum_tau w C^imp_d = improved chi_m, sum_tau w C^imp_d cos(2 pi tau / M_d) = improved F_d (structure reference)"""
    L = slm.Level(Mt, Mx, rot, beta)
    info = _update(L, 11 + Mx, regime)
    a, lab = info["a"], info["labels"]
    Ct, Cx = cref.split(scr.improved(L, a, lab)[None, :], Mt, Mx)
    chi = LD(3) * sum(LD(sa) ** 2 for sa in (np.asarray(a, dtype=np.float64).astype(LD)[lab == c].sum() for c in np.unique(lab))) / LD(L.n)
    assert abs(float(chi) - info["improved"]) <= 1e-9 * info["improved"]
    for d, (C, M) in enumerate(((Ct[0], Mt), (Cx[0], Mx))):
        w = cref.weights(M).astype(LD)
        cos = np.array([c for c in ssr.phases(slm.Level(M, M, False), 0)[0][:M // 2 + 1]], dtype=LD)  # cos(2 pi tau / M), exact on the axes
        assert abs((w * C).sum() - chi) <= 1e-15 * max(1.0, float(chi)), (d, (w * C).sum(), chi)
        F = ssr.improved(L, a, lab, d)
        assert abs((w * C * cos).sum() - F) <= 1e-15 * max(1.0, float(chi)), (d, (w * C * cos).sum(), F)


def _few_clusters(L, most=12):
    for seed in range(1, 400):
        phi = slm.sweep_draw(L, slm.initialise(L, 1, seed), 10, 1, seed)[0]
        for step in range(4):
            new, info = slsw.dev_update(L, phi, seed, 0, step)
            if 2 <= info["clusters"] <= most and np.bincount(info["labels"]).max() > 1:
                return info
            phi = new
    raise AssertionError("no update with few clusters")


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("Mt,Mx", [(2, 2), (2, 6), (4, 4)])
def test_improved_equals_the_mean_over_all_coin_assignments(Mt, Mx, rot):
    if L_n(Mt, Mx, rot) <= 12:                       # every vertex may be its own cluster: any update will do
        L = slm.Level(Mt, Mx, rot, 1.0)
        info = _update(L, 5, "mixed")
    else:
        L = slm.Level(Mt, Mx, rot, 2.0)
        info = _few_clusters(L)
    assert len(np.unique(info["labels"])) <= 12
    got, want = scr.improved(L, info["a"], info["labels"]), scr.coin_mean(L, info["a"], info["labels"])
    assert np.all(np.abs(got - want) <= 1e-15), (got, want)


def L_n(Mt, Mx, rot):
    return Mt * Mx // 2 if rot else Mt * Mx


@pytest.mark.parametrize("regime,beta", REGIMES)
@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("Mt,Mx", LEVELS)
def test_no_cluster_contributes_at_a_lag_of_its_width_or_beyond(Mt, Mx, rot, regime, beta):
    """The lemma behind the pair kernel's loop bound.  A link changes the slice index by at most 1 (mod M) on either geometry, so
    the slices a connected cluster occupies are an arc of the ring Z_M; two of them at circular distance tau <= M / 2 are joined by
    a walk inside the cluster that passes tau - 1 slices between them (either way round: M - tau >= tau), so the cluster occupies
    at least tau + 1 slices: with w_C occupied slices nothing contributes at tau >= w_C."""
    L = slm.Level(Mt, Mx, rot, beta)
    info = _update(L, 23 + Mt, regime)
    sizes = np.bincount(info["labels"])
    if regime == "singletons":
        assert (sizes == 1).any()
    if regime == "spanning":
        assert sizes.max() > L.n // 2
    widest = 0
    for d, M in enumerate((Mt, Mx)):
        for root, slices in scr.occupied(L, info["labels"], d).items():
            assert scr.largest_lag(slices, M) <= len(slices) - 1, (d, root, slices)
            widest = max(widest, len(slices))
    if regime == "spanning":
        assert widest == max(Mt, Mx)
    # and the model with the truncated loop is inside the bound of the full definition
    if L.n <= 600:
        got, want = scr.device_model(L, info["a"], info["labels"]), scr.improved(L, info["a"], info["labels"])
        assert np.all(np.abs(got - want.astype(np.float64)) <= scr.device_bound(L, info["a"], info["labels"]))


@pytest.mark.parametrize("n,collide", [(8, False), (64, False), (64, True), (37, True), (1, False)])
def test_the_slice_table_gives_the_integers_of_a_dict(n, collide):
    """insert order permuted, capacity exactly 2 n (n a power of two) and forced collisions (every key hashed to slot cap - 1, so
    the probe wraps round): the same sums, the same occupied-slice counts, whatever the order"""
    rng = random.Random(n)
    keys = rng.sample([(root, sl) for root in range(n) for sl in range(5)], n)       # a direction has at most n keys: all n here
    adds = [k + (rng.randrange(-2 ** 40, 2 ** 40),) for k in keys] + [rng.choice(keys) + (rng.randrange(-2 ** 40, 2 ** 40),) for _ in range(2 * n)]
    want, count = {}, {}
    for r, s, v in adds:
        if (r, s) not in want:
            count[r] = count.get(r, 0) + 1
        want[(r, s)] = want.get((r, s), 0) + v
    results = []
    for trial in range(3):
        rng.shuffle(adds)
        t = scr.SliceTable(n)
        if collide:
            t.hash_of = lambda key, cap=t.cap: cap - 1
        assert 2 * n <= t.cap < 4 * n and (n & (n - 1) or t.cap == 2 * n)
        for r, s, v in adds:
            t.add(r, s, v)
        assert t.items() == want and t.count == count
        assert all(t.lookup(r, s) == v for (r, s), v in want.items()) and t.lookup(n, 0) == 0
        if collide and len(want) > 1:
            assert t.probes > 0
        results.append((t.items(), t.count))
    assert results[0] == results[1] == results[2]


@pytest.mark.parametrize("rot", [False, True])
def test_the_device_model_does_not_depend_on_the_order_of_the_vertices(rot):
    L = slm.Level(6, 4, rot, 1.5)
    info = _update(L, 9, "mixed")
    order = list(range(L.n))
    base = scr.device_model(L, info["a"], info["labels"])
    for seed in range(3):
        random.Random(seed).shuffle(order)
        assert np.array_equal(scr.device_model(L, info["a"], info["labels"], order), base)


def test_the_scale_keeps_the_accumulator_inside_63_bits():
    for Mt, Mx, rot in [(2, 2, True), (16, 16, False), (1024, 1024, True), (1024, 1024, False), (32768, 32768, False), (2, 2 ** 29, False)]:
        L = slm.Level.__new__(slm.Level)
        L.Mt, L.Mx, L.rotated, L.n = Mt, Mx, rot, (Mt * Mx // 2 if rot else Mt * Mx)
        s = scr.scale_bits(L)
        n_slice = L.n // min(Mt, Mx)
        assert 0 <= s <= 32 and L.n * n_slice * 2 ** s + L.n <= 2 ** 63 - 1
        assert s == 32 or L.n * n_slice * 2 ** (s + 1) > 2 ** 62


def test_the_improved_correlator_has_the_mean_of_the_plain_one_on_a_model_chain():
    """4 x 4 unrotated, beta = 1, 32 chains x (100 + 400) updates of the model: per chain the mean over the run of (improved - plain
    C of the field before the update), every lag within 4.5 standard errors of zero, the error from the spread over the chains:
    the statistic of the GPU test, here on the model alone."""
    L = slm.Level(4, 4, False, 1.0)
    B, burn, meas = 32, 100, 400
    phi = slm.initialise(L, B, 71)
    diff = np.zeros((B, cref.n_out(4, 4)))
    for step in range(burn + meas):
        if step >= burn:
            plain = cref.correlator(4, 4, False, phi).astype(np.float64)
            for b in range(B):
                _, info = slsw.dev_update(L, phi[b], 72, b, step)
                diff[b] += scr.improved(L, info["a"], info["labels"]).astype(np.float64) - plain[b]
        phi, _ = slsw.dev_update_batch(L, phi, 72, 0, step)
    diff /= meas
    for k in range(diff.shape[1]):
        zcheck(f"sigma SW model 4x4 beta=1: improved - plain C[{k}]", float(diff[:, k].mean()), float(diff[:, k].std(ddof=1) / math.sqrt(B)),
               0.0, gate=4.5)
