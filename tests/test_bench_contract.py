"""The JSON line bench.py prints (the driver's contract): checked on the committed line of the final build, so that a
change of bench.py that drops or renames a field shows up without a GPU."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tag():
    return open(os.path.join(ROOT, "profiles", "FINAL")).read().strip()   # tag of the round's final build, e.g. "r02"


def _latest_default_line():
    return json.load(open(os.path.join(ROOT, "profiles", f"{_tag()}_bench.json")))


def test_bench_line_has_the_contract_fields():
    r = _latest_default_line()
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in r, key
    assert r["metric"] == "lattice-site-updates/sec" and r["higher_is_better"] is True and r["scaling"] == "weak"
    assert r["vs_baseline"] is None and r["dtype"] == "f64" and r["data"] == "synthetic"
    assert "workload" in r["config"] and "model" not in r["config"]
    roof = r["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in roof, key
    # r04 lines called a vector-issue-bound launch "valu" in the contract fields; from r05 (schema 2) bound / achieved / peak /
    # unit / frac are the measured HBM model in every line and the issue model sits under roofline.valu
    if _tag() >= "r05":
        assert roof["schema"] == 2 and roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["peak"] == 8000.0
        assert abs(roof["frac"] - roof["hbm_frac"]) < 1e-12
        if roof.get("limited_by") == "valu" and "valu" in roof:
            v = roof["valu"]
            assert 0.0 < v["frac"] <= 1.0 and v["unit"] == "Gcycle/s" and "NOT measured in this run" in v["note"]
    assert roof["bound"] in ("hbm", "mfma", "valu") and roof["unit"] in ("GB/s", "TFLOP/s", "Gcycle/s")
    if roof["bound"] == "valu":
        assert roof["unit"] == "Gcycle/s" and abs(roof["frac"] - roof["issue_frac"]) < 1e-12 and 0.0 < roof["hbm_frac"] <= 1.0
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-9
    assert 0.0 < roof["frac"] <= 1.0, "a roofline fraction above 1 says the byte model is not a bound"
    # the roofline names the kernel with the largest share of the step, and says what binds it
    shares = {k["kernel"]: k["share_of_step"] for k in r["kernels"] if "sweep" in k["role"] and "record_sample" not in k["role"]}
    assert roof["kernel"].startswith(max(shares, key=shares.get))
    for k in r["kernels"]:
        assert 0.0 < k["hbm_frac"] <= 1.0 and (k.get("valu_frac") is None or k["valu_frac"] <= 1.0)
        if k["traffic"] is not None:
            assert k["traffic"] >= 0.95 * k["hbm_floor_bytes_per_launch"]   # measured HBM bytes cannot undercut the floor
    assert set(r["step_includes"]) == {"sampler->draw", "qoi->evaluate", "stats->record_sample"}
    assert r["single_chain"]["chains_per_gpu"] == 1 and r["chains_128"]["chains_per_gpu"] == 128
    assert 0.0 < r["whole_step"]["hbm_floor_frac"] <= 1.0
    cpu = r["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in cpu, key
    assert cpu["kind"] in ("reference", "port")
    # value = units of all ranks / time
    assert abs(r["value"] * r["ms_per_step"] * 1e-3 / (2 * 1024 * 1024 * 11 * r["config"]["chains_total"]) - 1.0) < 1e-6
    # r03: the communicator record (null on one rank), the C++ path beside the Python-driven one, the cost-weighted issue bound
    assert "rccl" in r and r["rccl"] is None and r["n_gpus"] == 1
    cxx = r["cxx_path"]
    assert abs(cxx["over_python_driven"] - 1.0) < 0.07 and cxx["single_chain"]["chains_per_gpu"] == 1
    for k in r["kernels"]:
        if "issue_frac" in k:
            assert 0.0 < k["issue_frac"] <= k["valu_frac"] + 1e-9 <= 1.0 + 1e-9 and "profile" in k["valu_from"]


def test_multi_rank_lines_name_their_communicator():
    """The N = 2 rehearsals on the one-GPU box (gloo, ranks share the device): the line must say what exchanged the statistics
    and how many ranks it saw -- and that it was not RCCL."""
    for f in ("bench_n2_gloo_rehearsal", "bench_mlmc_n2_gloo_rehearsal"):
        r = json.load(open(os.path.join(ROOT, "profiles", f"{_tag()}_{f}.json")))
        assert r["n_gpus"] == 2 and r["rccl"]["ranks"] == 2 and r["rccl"]["allreduce_check"] == r["rccl"]["expected"] == 1.0
        assert r["rccl"]["lib"] is None and "NOT an RCCL run" in r["rccl"]["rehearsal"] and "gloo" in r["stats_collective"]


def test_bench_source_keeps_the_oracle_out_of_the_timed_path():
    src = open(os.path.join(ROOT, "bench.py")).read()
    # the oracle is only reached through the cpu_baseline subprocess
    assert "import oracle" not in src and "from oracle" not in src
    assert "cpu_baseline.py" in src


def test_secondary_workloads_report_fractions_of_real_bounds():
    """BASELINE configs 2, 3, 5 and the other workloads: committed lines of the final build; no fraction above 1, the
    register-resident HMC kernels carry a vector-issue fraction from the SQ counters of the same kernel build."""
    for w in ("gff", "rotor_hmc", "quartic_hmc", "ho_hmc", "quartic_mlmc", "quartic_mlmc_hier", "rotor_sweep"):
        r = json.load(open(os.path.join(ROOT, "profiles", f"{_tag()}_bench_{w}.json")))
        assert 0.0 < r["roofline"]["frac"] <= 1.0, w
        assert r["roofline"].get("valu_frac") is None or 0.0 < r["roofline"]["valu_frac"] <= 1.0, w
        if w.endswith("hmc") or w.startswith("quartic_mlmc"):
            assert r["roofline"]["limited_by"] == "valu" and r["roofline"]["valu_frac"] is not None, w
        if _tag() >= "r05":
            assert r["roofline"]["schema"] == 2 and r["roofline"]["bound"] == "hbm" and r["roofline"]["unit"] == "GB/s", w


def test_config5_as_the_reference_runs_it_agrees_with_single_level_hmc():
    """quartic_mlmc_hier (sampler = 'hierarchical') and quartic_mlmc (direct samplers): both telescoping
    sums within 2 sigma of the single-level HMC estimate on the finest lattice taken in the hierarchical run."""
    h = json.load(open(os.path.join(ROOT, "profiles", f"{_tag()}_bench_quartic_mlmc_hier.json")))
    # a level whose two-level steps never accept must be named in the line, from r04 on
    hacc = h["mlmc"]["hierarchical_acceptance_rank0"]
    if _tag() >= "r04":
        assert h["mlmc"]["frozen_levels"] == sorted({int(k) for acc in hacc.values() for k, v in acc.items() if v == 0.0})
    ref = h["mlmc"]["run_to_epsilon"]["single_level_fine_hmc"]
    assert abs(ref["z"]) < 2.0 and h["mlmc"]["run_to_epsilon"]["reached"]
    d = json.load(open(os.path.join(ROOT, "profiles", f"{_tag()}_bench_quartic_mlmc.json")))
    z = (d["mlmc"]["estimate"] - ref["mean"]) / (d["mlmc"]["error"] ** 2 + ref["error"] ** 2) ** 0.5
    assert abs(z) < 2.0, z


def test_hierarchical_line_with_moving_chains():
    """r04: the second hierarchical line (T_final = M_lat / 32): no frozen level, every hierarchical sampler moves on every
    level -- the multilevel path at bench scale with chains that move.  Its distance from single-level HMC is recorded in the
    line and NOT gated: with the reference's ceil(2 tau_int) sub-sampling the delayed-acceptance scheme is biased at this
    acceptance rate, which is what the line documents."""
    if _tag() < "r04":
        return
    h = json.load(open(os.path.join(ROOT, "profiles", f"{_tag()}_bench_quartic_mlmc_hier_T1024.json")))
    assert h["mlmc"]["frozen_levels"] == []
    for acc in h["mlmc"]["hierarchical_acceptance_rank0"].values():
        assert all(v > 0.02 for v in acc.values()), acc
    assert "z" in h["mlmc"]["run_to_epsilon"]["single_level_fine_hmc"]
    if _tag() >= "r05":
        # r05: the z-score is a field of the line, with the evidence that a value beyond 2 sigma here is the reference's scheme
        # (reference-order CPU run + the GPU test that pins the device to the oracle's biased value); the line with frozen
        # levels (T_final = M / 8) stays gated at 2 sigma in test_config5_as_the_reference_runs_it_agrees_with_single_level_hmc
        m = h["mlmc"]
        assert m["z_vs_single_level"] == m["run_to_epsilon"]["single_level_fine_hmc"]["z"]
        assert "r05_hier_bias_reference_order_level0.json" in m["z_vs_single_level_note"] and "running ceil(2 tau_int)" in m["sub_sampling"]
        ev = json.load(open(os.path.join(ROOT, "profiles", "r05_hier_bias_reference_order_level0.json")))
        lv = ev["mlmc"][0]["levels"][0]
        assert lv["z_fine_vs_hmc"] < -10 and abs(lv["z_coarse_vs_hmc"]) < 3 and 0.05 < lv["feeding_sampler_acceptance"] < 0.2


def test_default_line_carries_the_r04_records():
    """hbm_bound_probes (which kernels of the path reach 60 % of the HBM roofline), fast_path_cliff, the binding bound"""
    if _tag() < "r04":
        return
    r = _latest_default_line()
    probes = {p["entry_point"]: p for p in r["hbm_bound_probes"]["probes"]}
    # (five since the closed form: the single overrelaxation sweep both ways -- the default launch and the register-block one)
    assert len(probes) == 5 and all(0.0 < p["frac_of_hbm_peak"] <= 1.0 for p in probes.values())
    assert sum(p["reaches_60_percent"] for p in probes.values()) >= 3
    for p in probes.values():
        if p["counter_bytes"] is not None:
            assert p["counter_bytes"] >= 0.95 * p["floor_bytes"]
    cliff = {p["point"]: p for p in r["fast_path_cliff"]}
    # (0.6: beta = 4 draws from the wrapped-Cauchy envelope, 0.66-0.68 of the headline since the overrelaxation got cheap)
    if _tag() >= "r05":
        # every point within 0.6 of the headline, or explained by the padding of its edge tiles (rate x padding within 0.75)
        assert {"1000 x 1000 (no tile divides it)", "130 x 70 (no tile divides it)"} <= set(cliff)
        # (the beta = 10 point: the wrapped-Cauchy instance of the one launch kept its rate, 610-630 G/s, through the round's
        # second session while the step-envelope headline went from 936 to 1080 G/s -- the closed-form map of the cells with
        # this sampler was built and measured 1 % slower, profiles/r05_ab_beta4_mapped_cells.txt -- so its ratio is ~0.58;
        # beta = 4 and 6 take the step envelope since the limit moved from 2 beta = 4 to 16)
        for p in cliff.values():
            if p["over_headline"] is not None:
                floor = 0.55 if p["point"].startswith("beta = 10") else 0.6
                assert p["over_headline"] > floor or p["over_headline"] * p["padding_factor"] > 0.75, p
        assert any(p["point"].startswith("beta = 4") and p["over_headline"] > 0.85 for p in cliff.values())
        assert any(p["point"].startswith("beta = 6") and p["over_headline"] > 0.7 for p in cliff.values())
        ro = r["random_order"]
        assert ro["slowdown"] > 1.0 and ro["random_order_true"]["value_per_gpu"] > 0
    assert len(cliff) >= 6 and all(p["over_headline"] is None or p["over_headline"] > (0.4 if _tag() >= "r05" else 0.6) for p in cliff.values()), cliff
    assert r["roofline"]["bound"] == ("hbm" if _tag() >= "r05" else "valu") and 0.0 < r["roofline"]["frac"] <= 1.0
    assert r["cpu_baseline"]["cores"] == min(r["cpu_baseline"]["cores_available"], r["cpu_baseline"]["cpu_quota"])


def test_traffic_json_is_tied_to_a_kernel_build():
    t = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
    builds = {e["build"] for sec in ("entries", "valu", "kernels_valu_busy") for e in t[sec]}
    assert len(builds) == 1 and None not in builds
    assert builds == {_latest_default_line()["kernel_build"]}


def test_bench_refuses_a_rank_count_it_did_not_run():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "spawn_ranks" in src and "sys.exit(2)" in src
    import subprocess, sys
    env = dict(os.environ, WORLD_SIZE="3", RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-cpu-baseline"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "started 3 rank" in r.stderr


def test_overrelaxation_launch_plan_mirrors_the_library():
    """bench.or_plan restates next_launch's launch depths (lattice2d.hip): register-block kernels take up to `fuse`
    sweeps per launch in launches of equal depth, the others launches of `fuse` and a remainder."""
    import bench
    assert bench.or_plan(10, 6, True) == [(5, 2)]
    assert bench.or_plan(12, 6, True) == [(6, 2)]
    assert bench.or_plan(7, 6, True) == [(4, 1), (3, 1)]
    assert bench.or_plan(10, 4, True) == [(4, 1), (3, 2)]
    assert bench.or_plan(10, 4, False) == [(4, 2), (2, 1)]
    assert bench.or_plan(3, 4, False) == [(3, 1)]
    assert bench.or_plan(0, 6, True) == []
    # Schwinger overrelaxation in closed form: up to 10 sweeps per launch, launches of equal depth
    assert bench.or_plan(10, 10, True) == [(10, 1)]
    assert bench.or_plan(13, 10, True) == [(7, 1), (6, 1)]
    assert bench.or_plan(23, 10, True) == [(8, 2), (7, 1)]
    for n in range(0, 40):
        for fuse in (1, 2, 4, 6):
            for blocks in (False, True):
                plan = bench.or_plan(n, fuse, blocks)
                assert sum(d * k for d, k in plan) == n and all(1 <= d <= fuse for d, _ in plan)


def test_overrelaxation_launch_plan_equals_the_librarys():
    """the same (n, fuse, blocks) triples against the planner itself (mlmcpi_lattice_sweep_plan; no device needed): GFF 128^2
    takes the register-block kernels, GFF 32^2 the generic ones, Schwinger 128^2 the closed form (fuse 10)"""
    import bench
    from mlmcpathintegral_amd import abi, ops
    gff = {True: abi.lattice_action(abi.GFF, 128, 128, mass=3.0), False: abi.lattice_action(abi.GFF, 32, 32, mass=3.0)}
    schw = abi.lattice_action(abi.SCHWINGER, 128, 128, beta=1.0)
    triples = [(10, 6, True), (12, 6, True), (7, 6, True), (10, 4, True), (10, 4, False), (3, 4, False), (0, 6, True),
               (10, 10, True), (13, 10, True), (23, 10, True)]
    triples += [(n, fuse, blocks) for n in range(0, 40) for fuse in (1, 2, 4, 6) for blocks in (False, True)]
    for n, fuse, blocks in triples:
        depths = [l["n_overrelax"] for l in ops.lattice_sweep_plan(schw if fuse == 10 else gff[blocks], 2, n, 0, fuse)]
        grouped = [(d, depths.count(d)) for d in sorted(set(depths), reverse=True)]   # (depths never rise along a draw)
        assert depths == sorted(depths, reverse=True) and grouped == bench.or_plan(n, fuse, blocks), (n, fuse, blocks, depths)


def test_default_line_says_what_the_headline_number_is():
    """r05: ms per draw, draws/s, the updates executed one by one, the equivalent-updates flag, the hash of
    the loaded library, no experiment build in a record run, per-rank rates."""
    if _tag() < "r05":
        return
    r = _latest_default_line()
    B = r["config"]["chains_total"]
    assert abs(r["ms_per_draw"] - r["ms_per_step"]) < 1e-12
    assert abs(r["draws_per_s"] * r["ms_per_draw"] * 1e-3 / B - 1.0) < 1e-9
    eq = r["equivalent_updates"]
    assert eq["value_counts_equivalent_updates"] is True and eq["executed_as_link_updates"] == {"overrelaxation": 0, "heat_bath": 1}
    assert abs(r["executed_updates_per_s"] * 11 / r["value"] - 1.0) < 1e-9
    assert r["cpu_baseline"]["closed_form_possible"] is True
    assert len(r["lib_sha256"]) == 64 and r["lib"].endswith("libmlmcpi_hip.so") and "variant" not in r and "not_a_record" not in r
    assert r["variant_libs_present"] == []
    assert r["value_per_gpu"] and abs(sum(r["value_per_gpu"]) / r["value"] - 1.0) < 1e-9
    cpu = r["cpu_baseline"]
    assert cpu["wall_s"] >= 15.0 and cpu["per_core_min"] <= cpu["per_core"] <= cpu["per_core_max"]


def test_bench_refuses_an_experiment_library():
    """bench.py must not print a record line from a MLMCPI_LIB_VARIANT build (exit 2 before anything touches the GPU)"""
    import subprocess
    import sys
    env = dict(os.environ, MLMCPI_LIB_VARIANT="nosuch")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--no-extra-points"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "MLMCPI_LIB_VARIANT" in p.stderr and p.stdout.strip() == ""
