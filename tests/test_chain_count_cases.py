"""CPU: the conditions the case table of tests/chain_count_cases.py has to meet before tests/test_chain_count_gpu.py can rely on it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chain_count_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def batched_exports():
    """every function of include/mlmcpi_hip.h with a `uint32_t B` parameter"""
    with open(os.path.join(ROOT, "include", "mlmcpi_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    found = re.findall(r"\bint\s+(mlmcpi_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    return sorted(name for name, args in found if re.search(r"\buint32_t\s+B\s*(,|$)", args.strip()))


def test_every_batched_export_is_in_the_table_or_excluded_by_name():
    exports = batched_exports()
    assert len(exports) > 80 and "mlmcpi_path_initialise" in exports and "mlmcpi_sigma_twolevel_draw" in exports, len(exports)
    covered = {s for c in cc.CASES for s in c.symbols}
    assert covered <= set(exports), sorted(covered - set(exports))
    assert not covered & set(cc.EXCLUSIONS), sorted(covered & set(cc.EXCLUSIONS))
    missing = [e for e in exports if e not in covered and e not in cc.EXCLUSIONS]
    assert not missing, f"exports with a batch size that no case runs and no exclusion names: {missing}"
    assert all(isinstance(r, str) and len(r) > 20 for r in cc.EXCLUSIONS.values())
    assert set(cc.EXCLUSIONS) <= set(exports)


def test_the_big_batch_leaves_a_partial_last_workgroup_for_every_packing():
    assert cc.B_EDGE == 65535 < 65536 < cc.B_BIG
    assert all(cc.B_BIG % p for p in cc.PACKINGS) and all(cc.B_EDGE % p for p in cc.PACKINGS)
    assert 0 < cc.SPLIT < cc.B_EDGE and all(cc.SPLIT % p == 0 for p in (4, 16, 64)) and (cc.B_BIG - cc.SPLIT) % 256
    packed = {c.rides for c in cc.CASES if "/" in c.rides}
    assert packed == {"x/4", "x/64", "x/256", "y/16"}, packed
    assert {int(r.split("/")[1]) for r in packed} <= set(cc.PACKINGS)
    assert cc.pins(cc.B_BIG) == [0, 1, 65534, 65535, 65536, cc.B_BIG - 1] and cc.pins(cc.B_EDGE) == [0, 1, 65534] and cc.pins(1) == [0]


def test_outcomes_above_the_edge_follow_the_measurement():
    """the runtime takes gridDim.y > 65535 and every chain is right: only the units that refuse by name refuse"""
    assert cc.Y_ABOVE == "takes"
    refusing = {c.op for c in cc.CASES if c.above == "refuses"}
    assert refusing == {"path_sweep_draw", "sigma_level_maps", "sigma_level_draws", "sigma_level_transfers", "sigma_level_correlator",
                        "sigma_twolevel"}
    for c in cc.CASES:
        sizes = cc.batch_sizes(c)
        assert cc.B_EDGE in sizes if c.rides[0] in "yz" else sizes == [cc.B_BIG], c
        assert (cc.B_BIG in sizes) == (c.above == "takes"), c
        assert c.kind in ("map", "draw") and (c.split == "bits" or 0 < c.split <= 2e-10), c
    assert len(set(cc.IDS)) == len(cc.IDS)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_no_case_allocates_more_than_the_cap(case):
    assert cc.case_bytes(case, cc.B_BIG) <= cc.CAP_BYTES, (case, cc.case_bytes(case, cc.B_BIG))


def _query(name, *args):
    from mlmcpathintegral_amd import abi
    n = C.c_size_t(0)
    abi.call(name, *args, C.byref(n))
    return n.value


def test_workspace_queries_stay_inside_what_the_table_declares():
    """the host-only _workspace_bytes calls at B_BIG against the `work` column (path HMC at nt = 4, as the GPU test runs it)"""
    from mlmcpathintegral_amd import abi
    B = cc.B_BIG
    kinds = {"schwinger": abi.SCHWINGER, "gff": abi.GFF, "sigma": abi.NONLINEAR_SIGMA}
    for c in cc.CASES:
        s, got = c.shape, []
        if c.op in ("path_hmc_draw", "path_hmc_run"):
            act = abi.path_action(cc.KINDS.index(s["kind"]), s["M"], s["M"] / 8.0)
            got.append(_query("mlmcpi_path_hmc_workspace_bytes", C.byref(act), B, 4))
        elif c.op == "path_twolevel":
            act = abi.path_action(cc.KINDS.index(s["kind"]), s["M"], s["M"] / 8.0)
            got.append(_query("mlmcpi_path_twolevel_workspace_bytes", C.byref(act), B))
        elif c.op == "lattice_random_sweep":
            act = abi.lattice_action(kinds[s["kind"]], s["Mt"], s["Mt"], 1.0, 1.0)
            got.append(_query("mlmcpi_lattice_random_sweep_workspace_bytes", C.byref(act), B))
        elif c.op in ("sigma_cluster_draw", "sigma_sw_draw"):
            act = abi.lattice_action(abi.NONLINEAR_SIGMA, s["Mt"], s["Mt"], 1.0)
            got.append(_query("mlmcpi_" + c.op.replace("_draw", "") + "_workspace_bytes", C.byref(act), B))
        elif c.op in ("sigma_level_cluster", "sigma_level_sw"):
            lv = abi.sigma_level(s["Mt"], s["Mt"], s["rotated"], 1.0)
            for sym in c.symbols:
                if sym.endswith("_workspace_bytes"):
                    got.append(_query(sym, C.byref(lv), B))
        for g in got:
            assert g <= B * c.work + 4096, (c, g, B * c.work)
    # the guarded host-only queries refuse above the edge, as their launches do
    lv = abi.sigma_level(4, 4, 0, 1.0)
    for sym in ("mlmcpi_sigma_twolevel_workspace_bytes", "mlmcpi_sigma_level_correlator_workspace_bytes"):
        assert _query(sym, C.byref(lv), cc.B_EDGE) > 0
        with pytest.raises(abi.MlmcpiError):
            _query(sym, C.byref(lv), cc.B_EDGE + 1)


def test_inputs_belong_to_their_chains_and_carry_the_spikes():
    for kind in cc.KINDS:
        x = cc.path_input(kind, 4)
        sites, values = cc.path_spikes(kind, 4)
        assert x.shape == (cc.B_BIG, 4) and len({x[b].tobytes() for b in range(0, cc.B_BIG, 997)}) == len(range(0, cc.B_BIG, 997))
        for b in cc.spike_chains(cc.B_BIG):
            if kind == "rotor":   # a spike may have been moved off the cut, 0.05 at a time
                assert np.all(np.abs(x[b, sites] - values) <= 0.05 * 40 + 1e-12), (kind, b)
            else:
                assert (x[b, sites] == values).all() and np.abs(x[b]).max() > 6.0 > np.abs(x[2]).max(), (kind, b)
    import lattice_reference as lr
    th = cc.lattice_input("schwinger", 2)
    assert float(lr.distance_to_branch_cut(th, 2, 2).min()) >= 1e-5
    import path_reference as pr
    assert float(pr.distance_to_branch_cut(cc.path_input("rotor", 8)).min()) >= 1e-5


@pytest.mark.parametrize("kind", ["schwinger", "gff"])
def test_the_oracle_copies_on_one_tall_lattice_are_the_copies_chain_by_chain(orc, kind):
    """what ref_lattice_transfers of the GPU test relies on, at the chains around the edge"""
    tall, single = cc.lattice_transfers_oracle(kind, 4, 65530, 8, True), cc.lattice_transfers_oracle(kind, 4, 65530, 8, False)
    assert set(tall) == set(single) and all(np.array_equal(tall[k], single[k]) for k in tall)
    assert not np.array_equal(tall["coarse22"][0], tall["coarse22"][1])


def test_spike_chains_of_the_sigma_and_plain_inputs():
    for x in (cc.lattice_input("sigma", 2), cc.level_input(4, 1)):
        for b in cc.spike_chains(cc.B_BIG):
            assert list(x[b, :2]) + list(x[b, -2:]) == cc.SIGMA_SPIKES
    y = cc.plain_input(16, 50)
    assert all(y[b, 0] == 6.0 and y[b, -1] == -6.25 for b in cc.spike_chains(cc.B_BIG)) and np.abs(y[2]).max() < 1.0


def test_the_windowed_state_restatement_is_the_oracles_statistics(orc):
    rng = np.random.default_rng(3)
    series = rng.normal(0.3, 1.0, (7, 5))
    state = cc.window_state(series, 3)
    for b in range(5):
        st = orc.Statistics(3)
        for q in series[:, b]:
            st.record(q)
        n, avg, S = st.sums()
        assert state[b, 0] == n == 7 and abs(float(state[b, 1]) - avg) < 1e-14 and np.max(np.abs(state[b, 2:5].astype(float) - S)) < 1e-13
    assert state[0, 5] == 7 % 3 and set(state[0, 6:9].astype(float)) == set(series[4:, 0])
