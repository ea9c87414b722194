#!/usr/bin/env python3
"""Generates tests/golden/compiled_reference.json: what the reference's own Lattice1D / Lattice2D / Statistics /
parallel_mt19937_64 classes return, compiled unmodified into oracle/_ref/libref.so (oracle/Makefile, oracle/ref_wrap.cc),
for exactly the inputs the CPU tests feed the product and the oracle.  The fixture holds numbers only; the tests compare
against it, so they need neither the reference sources nor oracle/_ref.

    python tests/golden/make_compiled_reference_fixture.py           # needs oracle/_ref/libref.so (build() where the
                                                                     # reference sources are present)
    python tests/golden/make_compiled_reference_fixture.py --check   # re-runs the reference, compares with the file

Inputs: the sample streams are the tests' own (test_abi_host._ar1_series, test_stats_exchange._samples), imported from the
test modules; every stream is recorded with the SHA-256 of its bytes, and the tests check that digest before they compare.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
OUT = os.path.join(HERE, "compiled_reference.json")
sys.path.insert(0, TESTS)
sys.path.insert(0, ROOT)

# the cases of the tests that read this file
INDEX_MAP_CTYPES = (0, 1, 2, 3, 4)                 # test_abi_host.test_index_maps_match_compiled_reference (16 x 8)
LATTICE1D_M = (2, 7, 128)                          # test_abi_host.test_lattice1d_matches_compiled_reference
VERTEX_LIST_CASES = ((8, 4, 0), (8, 4, 1), (16, 4, 0), (16, 4, 1), (8, 0, 0), (4, 4, 0), (32, 4, 1))  # test_gff_levels
STATS_SINGLE = ((20, 0, 500), (20, 100, 700), (7, 3, 40), (100, 50, 3000))        # (k_max, nburn, n), seed 3, one rank
STATS_RANKS = ((2, 20, 0, 600), (2, 20, 40, 801), (3, 10, 5, 500), (4, 20, 10, 1000))  # (world, k_max, nburn, n), seed 11
RANK_SEEDS = (21172817, 2481317, 8923759, 5)       # test_stats_exchange.test_rank_seeding_matches_compiled_reference


def digest(q):
    return hashlib.sha256(np.ascontiguousarray(q, dtype=np.float64).tobytes()).hexdigest()


def stats_key(seed, n, world, rank, k_max, nburn):
    return f"seed={seed} n={n} world={world} rank={rank} k_max={k_max} nburn={nburn}"


def load_ref():
    path = os.path.join(ROOT, "oracle", "_ref", "libref.so")
    if not os.path.exists(path):
        sys.exit("oracle/_ref/libref.so not built: run build() where the reference sources are present")
    lib = C.CDLL(path)
    vp = C.c_void_p
    for f, res, args in (
            ("ref_lattice2d_new", vp, [C.c_uint, C.c_uint, C.c_int, C.c_int]), ("ref_lattice2d_coarse", vp, [vp]),
            ("ref_lattice2d_free", None, [vp]), ("ref_lattice2d_Mt", C.c_uint, [vp]), ("ref_lattice2d_Mx", C.c_uint, [vp]),
            ("ref_lattice2d_rotated", C.c_uint, [vp]), ("ref_lattice2d_nvertices", C.c_uint, [vp]),
            ("ref_vertex_cart2lin", C.c_uint, [vp, C.c_int, C.c_int]),
            ("ref_link_cart2lin", C.c_uint, [vp, C.c_int, C.c_int, C.c_int]),
            ("ref_link_lin2cart", None, [vp, C.c_uint, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
            ("ref_lattice2d_neighbours", None, [vp, vp]), ("ref_lattice2d_n_fineonly", C.c_uint, [vp]),
            ("ref_lattice2d_n_coarse", C.c_uint, [vp]), ("ref_lattice2d_fineonly", None, [vp, vp]),
            ("ref_lattice2d_fine2coarse", None, [vp, vp]),
            ("ref_lattice1d_neighbours", None, [C.c_uint, C.c_double, vp, C.POINTER(C.c_double)]),
            ("ref_stats_new", vp, [C.c_uint]), ("ref_stats_free", None, [vp]), ("ref_stats_record", None, [vp, vp, C.c_uint]),
            ("ref_stats_reset", None, [vp, C.c_int]), ("ref_stats_get", None, [vp, vp]), ("ref_stats_autocorr", None, [vp, vp]),
            ("ref_parallel_mt19937_64", None, [C.c_ulonglong, C.c_uint, vp])):
        getattr(lib, f).restype = res
        getattr(lib, f).argtypes = args
    return lib


def index_maps(ref, ctype):
    """every level of the coarsening hierarchy of a 16 x 8 lattice: neighbour table, vertex map, link map (unrotated)"""
    levels = []
    h = ref.ref_lattice2d_new(16, 8, ctype, 0)
    while h:
        Mt, Mx, rot = ref.ref_lattice2d_Mt(h), ref.ref_lattice2d_Mx(h), ref.ref_lattice2d_rotated(h)
        nb = np.zeros(ref.ref_lattice2d_nvertices(h) * 8, dtype=np.uint32)
        ref.ref_lattice2d_neighbours(h, nb.ctypes.data_as(C.c_void_p))
        vertex, link = [], []
        for i in range(-2, Mt + 2):
            for j in range(-2, Mx + 2):
                if rot and (i + j) % 2:
                    continue
                vertex.append([i, j, ref.ref_vertex_cart2lin(h, i, j)])
                if not rot:
                    link += [[i, j, mu, ref.ref_link_cart2lin(h, i, j, mu)] for mu in (0, 1)]
        levels.append({"Mt": Mt, "Mx": Mx, "rotated": rot, "neighbours": nb.tolist(), "vertex_cart2lin": vertex,
                       "link_cart2lin": link})
        nxt = ref.ref_lattice2d_coarse(h)
        ref.ref_lattice2d_free(h)
        h = nxt
    return levels


def lattice1d(ref, M):
    nb = np.zeros(2 * M, dtype=np.uint32)
    a = C.c_double()
    ref.ref_lattice1d_neighbours(M, 4.0, nb.ctypes.data_as(C.c_void_p), C.byref(a))
    return {"neighbours": nb.tolist(), "a_lat": a.value}


def vertex_lists(ref, Mt, ctype, level):
    h = ref.ref_lattice2d_new(Mt, Mt, ctype, level)
    f = np.zeros(ref.ref_lattice2d_n_fineonly(h), dtype=np.uint32)
    p = np.zeros(2 * ref.ref_lattice2d_n_coarse(h), dtype=np.uint32)
    ref.ref_lattice2d_fineonly(h, f.ctypes.data_as(C.c_void_p))
    ref.ref_lattice2d_fine2coarse(h, p.ctypes.data_as(C.c_void_p))
    ref.ref_lattice2d_free(h)
    return {"fineonly": f.tolist(), "fine2coarse": p.tolist()}


def link_maps(ref, pins):
    """link_cart2lin / link_lin2cart of Lattice2D(m, m) at the points of tests/golden/schwinger_ref_python.json"""
    out = {}
    for case in pins["schwinger"]:
        if case["cart2lin"] is None:
            continue
        m = case["m"]
        h = ref.ref_lattice2d_new(m, m, 0, 0)
        c2l = [[i, j, mu, ref.ref_link_cart2lin(h, i, j, mu)] for i, j, mu, _ in case["cart2lin"] + case["cart2lin_wrapped"]]
        l2c = []
        for ell, _, _, _ in case["lin2cart"]:
            ci, cj, cm = C.c_int(), C.c_int(), C.c_int()
            ref.ref_link_lin2cart(h, ell, C.byref(ci), C.byref(cj), C.byref(cm))
            l2c.append([ell, ci.value, cj.value, cm.value])
        ref.ref_lattice2d_free(h)
        out[str(m)] = {"cart2lin": c2l, "lin2cart": l2c}
    return out


def stats_run(ref, q, k_max, nburn, reset_at=None):
    """one reference Statistics fed q: burn-in of nburn samples, soft reset (montecarlosinglelevel.cc:27-37), the rest"""
    h = ref.ref_stats_new(k_max)
    q = np.ascontiguousarray(q, dtype=np.float64)
    if nburn and nburn <= q.size:
        ref.ref_stats_record(h, q[:nburn].ctypes.data_as(C.c_void_p), nburn)
        ref.ref_stats_reset(h, 0)
        rest = np.ascontiguousarray(q[nburn:])
    else:
        rest = q
    if rest.size:
        ref.ref_stats_record(h, rest.ctypes.data_as(C.c_void_p), rest.size)
    out, ck = np.zeros(6), np.zeros(k_max)
    ref.ref_stats_get(h, out.ctypes.data_as(C.c_void_p))
    ref.ref_stats_autocorr(h, ck.ctypes.data_as(C.c_void_p))
    ref.ref_stats_free(h)
    return {"input_sha256": digest(q), "get": out.tolist(), "autocorr": ck.tolist()}


def generate():
    from test_abi_host import _ar1_series
    from test_stats_exchange import _samples
    ref = load_ref()
    with open(os.path.join(HERE, "schwinger_ref_python.json")) as f:
        pins = json.load(f)
    stats = {}
    for k_max, nburn, n in STATS_SINGLE:
        stats[stats_key(3, n, 1, 0, k_max, nburn)] = stats_run(ref, _samples(n, seed=3), k_max, nburn)
    for world, k_max, nburn, n in STATS_RANKS:
        q = _samples(n, seed=11)
        for r in range(world):
            stats[stats_key(11, n, world, r, k_max, nburn)] = stats_run(ref, q[r::world], k_max, nburn)
    mt = {}
    for seed in RANK_SEEDS:
        v = np.zeros(8, dtype=np.uint64)
        ref.ref_parallel_mt19937_64(seed, 8, v.ctypes.data_as(C.c_void_p))
        mt[str(seed)] = [int(x) for x in v]
    q = _ar1_series()   # Statistics(20): 1000 samples, soft reset, 4000 samples
    return {
        "_provenance": "tests/golden/make_compiled_reference_fixture.py: outputs of the reference's Lattice1D, Lattice2D, "
                       "Statistics and parallel_mt19937_64, compiled unmodified (oracle/_ref/libref.so); numbers only",
        "index_maps_16x8": {str(c): index_maps(ref, c) for c in INDEX_MAP_CTYPES},
        "lattice1d_T4": {str(M): lattice1d(ref, M) for M in LATTICE1D_M},
        "vertex_lists": {f"{Mt} {c} {lv}": vertex_lists(ref, Mt, c, lv) for Mt, c, lv in VERTEX_LIST_CASES},
        "link_maps": link_maps(ref, pins),
        "statistics_ar1": stats_run(ref, q, 20, 1000),
        "statistics": stats,
        "parallel_mt19937_64": mt,
    }


if __name__ == "__main__":
    data = generate()
    if "--check" in sys.argv:
        with open(OUT) as f:
            ok = json.load(f) == json.loads(json.dumps(data))
        print("compiled_reference.json matches the reference" if ok else "compiled_reference.json DIFFERS from the reference")
        sys.exit(0 if ok else 1)
    with open(OUT, "w") as f:
        json.dump(data, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
