"""long double reference of the cluster-improved time-slice correlator of the Swendsen-Wang update (sigma_sw.hip,
mlmcpi_sigma_level_sw_correlator_draw), built on the labels and a = r . sigma that sigma_sw_model.dev_update and
sigma_level_sw_model.dev_update return, and a Python statement of the device's slice table and fixed-point arithmetic.

A level vertex sits at (i, j) (sigma_correlator_reference.coords), direction 0 = t has x_0 = i, M_0 = Mt, direction 1 = x has
x_1 = j, M_1 = Mx.  Per cluster C, direction d and slice i

  P_C,d(i)     = sum_{l in C, x_d(l) = i} a_l
  C_d^imp(tau) = (3 / n) sum_C sum_{i < M_d} P_C,d(i) P_C,d((i + tau) mod M_d),   tau = 0 .. M_d / 2

in the layout of the plain correlator, [n_out] with C_t first.  It is the mean over the coins (each cluster's sign) of
3 (r . S'_i)(r . S'_{i + tau}) / n summed over i: the cross terms of two clusters vanish; the mean over r of (r . u)(r . v) is u . v / 3.
"""
import itertools

import numpy as np

import sigma_correlator_reference as ref

LD = np.longdouble
FIX = 2.0 ** 32
MASK64 = (1 << 64) - 1


def entries(L, a, labels, d):
    """the occupied (cluster, slice) pairs of direction d, sorted by key = root M + slice: (keys, P long double, sum |a| float,
    number of vertices)"""
    M = (L.Mt, L.Mx)[d]
    x = ref.coords(L.Mt, L.Mx, L.rotated)[d]
    key = np.asarray(labels, dtype=np.int64) * M + x
    keys, inv = np.unique(key, return_inverse=True)
    a = np.asarray(a, dtype=np.float64)
    P, S, cnt = np.zeros(len(keys), dtype=LD), np.zeros(len(keys)), np.zeros(len(keys), dtype=np.int64)
    np.add.at(P, inv, a.astype(LD))
    np.add.at(S, inv, np.abs(a))
    np.add.at(cnt, inv, 1)
    return keys, P, S, cnt


def _partners(keys, M, tau):
    """for every entry (C, i) the index of (C, (i + tau) mod M) among the entries, and whether it exists"""
    root, sl = keys // M, keys % M
    want = root * M + (sl + tau) % M
    idx = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
    return idx, keys[idx] == want


def improved_direction(L, a, labels, d):
    M = (L.Mt, L.Mx)[d]
    keys, P, _, _ = entries(L, a, labels, d)
    out = np.zeros(M // 2 + 1, dtype=LD)
    for tau in range(M // 2 + 1):
        idx, hit = _partners(keys, M, tau)
        out[tau] = (P[hit] * P[idx[hit]]).sum()
    return LD(3) * out / LD(len(a))


def improved(L, a, labels):
    """C^imp [n_out], C_t first, long double"""
    return np.concatenate([improved_direction(L, a, labels, d) for d in range(2)])


def brute_force(L, a, labels):
    """the definition with no bookkeeping at all: a loop over clusters, slices and lags (small levels)"""
    out = []
    a = np.asarray(a, dtype=np.float64).astype(LD)
    for d, M in enumerate((L.Mt, L.Mx)):
        x = ref.coords(L.Mt, L.Mx, L.rotated)[d]
        C = np.zeros(M // 2 + 1, dtype=LD)
        for root in np.unique(labels):
            P = np.array([a[(labels == root) & (x == i)].sum() for i in range(M)], dtype=LD)
            for tau in range(M // 2 + 1):
                C[tau] += sum(P[i] * P[(i + tau) % M] for i in range(M))
        out.append(LD(3) * C / LD(len(a)))
    return np.concatenate(out)


def coin_mean(L, a, labels):
    """the mean over ALL coin assignments of (3 / n) sum_i (sum_l s_C(l) a_l [x_d = i]) (the same at i + tau), by enumeration"""
    roots = list(np.unique(labels))
    assert len(roots) <= 12
    a = np.asarray(a, dtype=np.float64).astype(LD)
    tot = np.zeros(ref.n_out(L.Mt, L.Mx), dtype=LD)
    for signs in itertools.product((1, -1), repeat=len(roots)):
        sa = a * np.array([signs[roots.index(c)] for c in labels], dtype=LD)
        row = []
        for d, M in enumerate((L.Mt, L.Mx)):
            x = ref.coords(L.Mt, L.Mx, L.rotated)[d]
            S = np.array([sa[x == i].sum() for i in range(M)], dtype=LD)
            row.append(np.array([sum(S[i] * S[(i + tau) % M] for i in range(M)) for tau in range(M // 2 + 1)], dtype=LD))
        tot += np.concatenate(row)
    return LD(3) * tot / LD(2 ** len(roots)) / LD(len(a))


def occupied(L, labels, d):
    """{root: sorted slices of direction d the cluster has a vertex in}"""
    x = ref.coords(L.Mt, L.Mx, L.rotated)[d]
    out = {}
    for root, sl in zip(np.asarray(labels).tolist(), np.asarray(x).tolist()):
        out.setdefault(root, set()).add(sl)
    return {root: sorted(s) for root, s in out.items()}


def largest_lag(slices, M):
    """the largest tau <= M / 2 at which a cluster with these slices contributes: the largest circular distance of two of them"""
    s = np.asarray(slices)
    dist = np.abs(s[:, None] - s[None, :])
    return int(np.minimum(dist, M - dist).max())


# ---- the device's arithmetic, restated ------------------------------------------------------------------------------------------
def scale_bits(L):
    """s of the accumulators: min(32, 62 - ceil(log2(n n_slice))), n_slice = n / min(Mt, Mx) the vertices of the larger slice"""
    bound, lb = L.n * (L.n // min(L.Mt, L.Mx)), 0
    while (1 << lb) < bound:
        lb += 1
    return min(32, 62 - lb)


class SliceTable:
    """the open-addressing table of one chain and direction: 2^lg >= 2 n slots, key (root << 32) | (slice + 1), 0 = empty, linear
    probing from a multiplicative hash (`hash_of` may be replaced to force collisions); `count[root]` = slices the root occupies"""

    def __init__(self, n, hash_of=None):
        self.lg = 1
        while (1 << self.lg) < 2 * n:
            self.lg += 1
        self.cap = 1 << self.lg
        self.keys, self.vals, self.count = [0] * self.cap, [0] * self.cap, {}
        self.hash_of = hash_of or (lambda key: ((key * 0x9E3779B97F4A7C15) & MASK64) >> (64 - self.lg))
        self.probes = 0

    @staticmethod
    def key(root, sl):
        return (root << 32) | (sl + 1)

    def _slot(self, key, insert):
        slot = self.hash_of(key)
        for _ in range(self.cap):
            if self.keys[slot] == key:
                return slot
            if self.keys[slot] == 0:
                if not insert:
                    return None
                self.keys[slot] = key
                self.count[key >> 32] = self.count.get(key >> 32, 0) + 1
                return slot
            slot = (slot + 1) & (self.cap - 1)
            self.probes += 1
        raise AssertionError("a probe loop reached its cap")

    def add(self, root, sl, v):
        self.vals[self._slot(self.key(root, sl), True)] += v

    def lookup(self, root, sl):
        slot = self._slot(self.key(root, sl), False)
        return 0 if slot is None else self.vals[slot]

    def items(self):
        return {((k >> 32), (k & 0xFFFFFFFF) - 1): v for k, v in zip(self.keys, self.vals) if k}


def device_model(L, a, labels, order=None):
    """what the kernels compute, in their integers: q(a) = rint(a 2^32) into the tables (in the order `order` of the vertices),
    the terms rint(P P' 2^(s - 64)) with the product formed in double, for tau <= min(M / 2, w_C - 1) only, and
    (acc 2^-s) (3 / n) at the end.  [n_out] float64"""
    n, s = len(a), scale_bits(L)
    q = np.rint(np.asarray(a, dtype=np.float64) * FIX).astype(np.int64)
    order = range(n) if order is None else order
    out = []
    for d, M in enumerate((L.Mt, L.Mx)):
        x = ref.coords(L.Mt, L.Mx, L.rotated)[d]
        table = SliceTable(n)
        for l in order:
            table.add(int(labels[l]), int(x[l]), int(q[l]))
        acc = [0] * (M // 2 + 1)
        for (root, i), P in table.items().items():
            for tau in range(min(M // 2, table.count[root] - 1) + 1):
                Q = table.lookup(root, (i + tau) % M)
                acc[tau] += int(np.rint((float(P) * float(Q)) * 2.0 ** (s - 64)))
        out.append(np.array([(float(v) * 2.0 ** -s) * (3.0 / n) for v in acc]))
    return np.concatenate(out)


DELTA = 1.5 * 2.0 ** -32   # per vertex: 2^-33 for the rounding of q(a), 2^-32 where a libm ulp in a moves it (the structure test's)


def device_bound(L, a, labels):
    """absolute bound on |device C^imp - improved(...)| per lag, [n_out], from the roundings and nothing else.
    (1) The device's P~ is a sum of llrint(a 2^32): against the exact P it is off by at most delta_i = n_C(i) DELTA.  With S_i = the
    sum of |a| over the slice of the cluster, |P| <= S_i, so a product is off by S_i delta_j + S_j delta_i + delta_i delta_j.
    (2) The two integers are converted to double and multiplied: three roundings, then the conversion of the accumulator, 3 / n
    and the last product, three more: 8 x 2^-53 of (S_i + delta_i)(S_j + delta_j) covers them with room.
    (3) Every term is rounded to the accumulator's unit: 2^-(s + 1) per pair of occupied slices."""
    s, n = scale_bits(L), len(a)
    out = []
    for d, M in enumerate((L.Mt, L.Mx)):
        keys, _, S, cnt = entries(L, a, labels, d)
        delta = cnt * DELTA
        b = np.zeros(M // 2 + 1)
        for tau in range(M // 2 + 1):
            idx, hit = _partners(keys, M, tau)
            Si, Sj, di, dj = S[hit], S[idx[hit]], delta[hit], delta[idx[hit]]
            b[tau] = (Si * dj + Sj * di + di * dj).sum() + 8 * 2.0 ** -53 * ((Si + di) * (Sj + dj)).sum() + hit.sum() * 2.0 ** -(s + 1)
        out.append(3.0 * b / n)
    return np.concatenate(out)


def susceptibility_bound(L, a, labels):
    """absolute bound on |device improved chi_m - 3 sum_C A_C^2 / n|: sigma_sw_structure_reference.device_bound is written for the
    two sums (cos, sin) of a direction with |a w| <= |a|; the improved chi_m is one such sum with w = 1, so half of it"""
    import sigma_sw_structure_reference as ssr
    return 0.5 * ssr.device_bound(L, a, labels, 0)
