#!/usr/bin/env python3
"""Generates tests/golden/sigma_compactexp.json from the reference author's own Python wrapper of the heat-bath law of the
O(3) nonlinear sigma model.  Runs in the build container only (it imports /root/reference/tools/plot_distribution.py;
nothing of that file is copied: the fixture holds numbers).

    python tests/golden/make_sigma_fixture.py

What is imported and what it pins:
  * /root/reference/tools/plot_distribution.py
      CompactExpDistribution.f_analytical (:124-143) = CompactExpDistribution::evaluate (distribution/compactexpdistribution.cc),
      the density p(x) = s exp(s x) / (2 sinh s) on [-1, 1] of sigma . Delta^ in NonlinearSigmaAction::heatbath_update
      (action/qft/nonlinearsigmaaction.cc:24-72), s = beta |Delta|.
    Tabulated on 1001 points of [-1, 1] for every s of S_GRID.  s = 0 is not in the table: the wrapper's normalisation
    s / (2 sinh s) is 0 / 0 there (the test takes the limit, the uniform law).
"""
import importlib.util
import json
import os

os.environ.setdefault("MPLBACKEND", "Agg")
import numpy as np  # noqa: E402

REF = "/root/reference/tools"
HERE = os.path.dirname(os.path.abspath(__file__))
S_GRID = [1e-8, 0.1, 1.0, 4.0, 16.0, 40.0]


def load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    pd = load("plot_distribution")
    x = np.linspace(-1.0, 1.0, 1001)
    table = []
    for s in S_GRID:
        dist = pd.CompactExpDistribution(np.zeros(1), x, x, s)
        table.append({"s": s, "density": [float(v) for v in dist.f_analytical(x)]})
    out = {
        "_provenance": "tests/golden/make_sigma_fixture.py importing /root/reference/tools/plot_distribution.py "
                       "CompactExpDistribution.f_analytical",
        "x": [float(v) for v in x],
        "table": table,
    }
    with open(os.path.join(HERE, "sigma_compactexp.json"), "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
