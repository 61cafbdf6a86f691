"""The ADF kernels alone (gpumd_amd/csrc/nep_adf.h) through nepmi_adf_sample on synthetic configurations, in both tiers: the GPU
tier runs the cell binning + the persistent triplet kernel, the CPU tier (kernel emulator) the plain body over the same cell list,
the same mask rule and the same bin rule.

Expected counts: the definition restated in numpy over ALL triplets, in double -- minimum image through fractional coordinates; a
neighbour a of the centre i is in role J of a row if its type matches and rmin_j^2 <= d2 < rmax_j^2 (K likewise), the row counts
the unordered pair {a, b} once if (J(a) and K(b)) or (J(b) and K(a)); c = (r_ia . r_ib) / sqrt(d2_ia d2_ib) clamped,
theta = acos(c) 180 / pi, bin = min(floor(theta * inv), num_bins - 1), inv = 1.0 / (180.0 / num_bins).  A triplet is AMBIGUOUS if a
leg's d2 lies within a relative 1e-9 of a squared bound of a range it could belong to, or if moving c by +-1e-12 changes the bin;
every random case asserts first that it has none, so the integer counts are equal EXACTLY.  The lattice cases have integer
coordinates: every d2 is exact on both sides and so are the unit vectors along the axes.

Shapes (the smallest at which the kernel can go wrong): n in {2, 3, 63, 64, 65, 1000} (a wavefront is 64 lanes, a pass of a
workgroup four centre atoms; at n = 1000 a centre has about 210 members, several passes of the pair loop); a box of exactly 2.5 rc;
5 x 6 x 9 cells; a triclinic box; one and two free directions with atoms outside the box; all atoms in one eighth of the box
(a cell holds many atoms: one lane walks them); 7, 90 and 720 bins; rmin > 0; the triple form with the symmetric rule; a row whose
itype has no atom; 32 rows at 720 bins (90 KB of table: the form with global atomics) against the same rows in LDS; the capacity."""
import ctypes as C

import numpy as np
import pytest

import helpers as H

NEP = H.golden("PbTe", "nep.txt")
EPS_REL = 1e-9
DC = 1e-12


def global_rows(rmin, rmax):
    return [(-1, -1, -1, rmin, rmax, rmin, rmax)]


def bin_of(c, nb):
    """definition D"""
    inv = 1.0 / (180.0 / nb)
    theta = np.arccos(np.clip(c, -1.0, 1.0)) * 180.0 / np.pi
    return np.minimum(np.floor(theta * inv).astype(np.int64), nb - 1)


def expected_counts(pos, typ, h9, pbc, rows, nb, eps_rel=EPS_REL, delta=None):
    """all triplets -> (counts [M, nb], ambiguous [M, nb]); pos = [3, n].
    delta (a distance, A): the ambiguity rule of the run tests instead -- a leg within delta of a bound, an angle within
    (180 / pi) delta (1 / d_ia + 1 / d_ib) of a bin edge."""
    Hm = np.asarray(h9, dtype=np.float64).reshape(3, 3)
    s = np.linalg.solve(Hm, pos)
    n, M = pos.shape[1], len(rows)
    typ = np.asarray(typ)
    counts, amb = np.zeros((M, nb), dtype=np.int64), np.zeros((M, nb), dtype=np.int64)
    rcmax = max(max(r[4], r[6]) for r in rows)
    width = 180.0 / nb
    inv = 1.0 / width

    def near(d2, bound):
        if delta is None and eps_rel is None:  # exact coordinates: a leg ON a bound is decided by the closed / open rule
            return np.zeros(d2.shape, dtype=bool)
        if delta is None:
            return np.abs(d2 - bound * bound) <= eps_rel * bound * bound
        return np.abs(d2 - bound * bound) <= 2.0 * bound * delta + delta * delta

    reach2 = rcmax * rcmax * (1.0 + 1e-6) + (0.0 if delta is None else 4.0 * rcmax * delta)
    for i in range(n):
        ds = s - s[:, i:i + 1]
        for d in range(3):
            if pbc[d]:
                ds[d] -= np.round(ds[d])
        dv = Hm @ ds
        d2 = (dv * dv).sum(axis=0)
        d2[i] = 0.0
        cand = np.flatnonzero((d2 > 0.0) & (d2 <= reach2))
        if len(cand) < 2:
            continue
        t, q2, v = typ[cand], d2[cand], dv[:, cand]
        J, K = np.zeros(len(cand), dtype=np.uint32), np.zeros(len(cand), dtype=np.uint32)
        nJ, nK = np.zeros(len(cand), dtype=np.uint32), np.zeros(len(cand), dtype=np.uint32)
        for m, (it, jt, kt, j0, j1, k0, k1) in enumerate(rows):
            if it >= 0 and it != typ[i]:
                continue
            bit = np.uint32(1 << m)
            tj = np.ones(len(cand), dtype=bool) if jt < 0 else (t == jt)
            tk = np.ones(len(cand), dtype=bool) if kt < 0 else (t == kt)
            J[tj & (q2 >= j0 * j0) & (q2 < j1 * j1)] |= bit
            K[tk & (q2 >= k0 * k0) & (q2 < k1 * k1)] |= bit
            nJ[tj & (near(q2, j0) | near(q2, j1))] |= bit
            nK[tk & (near(q2, k0) | near(q2, k1))] |= bit
        keep = np.flatnonzero((J | K | nJ | nK) != 0)
        if len(keep) < 2:
            continue
        J, K, nJ, nK, q2, v = J[keep], K[keep], nJ[keep], nK[keep], q2[keep], v[:, keep]
        a, b = np.triu_indices(len(keep), 1)
        hit = (J[a] & K[b]) | (J[b] & K[a])
        # a pair one of whose legs sits on a bound: the rows it counts in, or would count in with the leg on the other side
        Jn, Kn = J | nJ, K | nK
        shaky = ((nJ[a] & Kn[b]) | (Jn[a] & nK[b]) | (nJ[b] & Kn[a]) | (Jn[b] & nK[a]))
        sel = np.flatnonzero((hit | shaky) != 0)
        if len(sel) == 0:
            continue
        a, b, hit, shaky = a[sel], b[sel], hit[sel], shaky[sel]
        c = np.clip((v[:, a] * v[:, b]).sum(axis=0) / np.sqrt(q2[a] * q2[b]), -1.0, 1.0)
        w = bin_of(c, nb)
        if delta is None:
            wlo, whi = bin_of(np.clip(c + DC, -1.0, 1.0), nb), bin_of(np.clip(c - DC, -1.0, 1.0), nb)
        else:
            theta = np.arccos(c) * 180.0 / np.pi
            tol = (180.0 / np.pi) * delta * (1.0 / np.sqrt(q2[a]) + 1.0 / np.sqrt(q2[b]))
            wlo = np.clip(np.floor((theta - tol) * inv).astype(np.int64), 0, nb - 1)
            whi = np.clip(np.floor((theta + tol) * inv).astype(np.int64), 0, nb - 1)
        for m in range(M):
            hm = ((hit >> np.uint32(m)) & np.uint32(1)) != 0
            if hm.any():
                np.add.at(counts[m], w[hm], 1)
            sm = ((shaky >> np.uint32(m)) & np.uint32(1)) != 0
            edge = (hm | sm) & (wlo != whi)
            for ws in (wlo, whi):
                if edge.any():
                    np.add.at(amb[m], ws[edge], 1)
            leg = sm & (wlo == whi)
            if leg.any():
                np.add.at(amb[m], w[leg], 1)
    return counts, amb


# ---- configurations: name -> (pos [3, n], typ, h9, pbc, rows, num_bins, T) --------------------------------------------------------
def _uniform(n, L, seed, pbc=(1, 1, 1), T=2, typ=None, spill=0.0, corner=1.0):
    rng = np.random.default_rng(seed)
    L = np.asarray(L, dtype=np.float64)
    pos = rng.uniform(0.0, 1.0, (3, n)) * (L * corner)[:, None]
    for d in range(3):
        if not pbc[d] and spill:
            pos[d] = rng.uniform(-spill, L[d] + spill, n)  # a free direction: atoms may lie outside the box
    if typ is None:
        typ = (np.arange(n) * 7 % T).astype(np.int32)  # interleaved membership
    return pos, np.asarray(typ, dtype=np.int32), np.diag(L).reshape(9), pbc


TRIPLE_ROWS = [(0, 1, 1, 0.0, 4.0, 0.0, 4.0),   # j == k, equal ranges
               (1, 0, 1, 0.0, 3.0, 1.0, 4.0),   # j != k
               (0, 0, 0, 0.0, 2.5, 2.0, 4.0)]   # j == k with DIFFERENT ranges: the symmetric rule
BOX = [10.4, 10.9, 11.3]


def _rows32():
    rows = []
    for it in (0, 1):
        for jt in (0, 1):
            for kt in (0, 1):
                for (j0, j1, k0, k1) in ((0.0, 4.0, 0.0, 4.0), (1.5, 3.0, 0.0, 4.0), (0.0, 3.0, 1.5, 4.0), (1.5, 4.0, 1.5, 3.0)):
                    rows.append((it, jt, kt, j0, j1, k0, k1))
    return rows


def _case(name):
    g = global_rows(0.0, 4.0)
    if name.startswith("n"):
        n = int(name[1:])
        pos, typ, h, pbc = _uniform(n, BOX, seed=100 + n)
        return pos, typ, h, pbc, g, 90, 2
    if name == "exactly_2p5_rc":
        pos, typ, h, pbc = _uniform(400, [10.0, 10.0, 10.0], seed=5)
        return pos, typ, h, pbc, g, 90, 2
    if name == "cells_5_6_9":
        pos, typ, h, pbc = _uniform(700, [2.6 * 4.0, 3.2 * 4.0, 4.7 * 4.0], seed=6)
        return pos, typ, h, pbc, g, 90, 2
    if name == "triclinic":
        h, typ, x = H.pbte_supercell((2, 2, 2), rattle=0.05, seed=4)
        return x.reshape(3, -1), typ, h, (1, 1, 1), g, 90, 2
    if name == "one_free":
        pos, typ, h, pbc = _uniform(500, [10.5, 11.0, 12.0], seed=7, pbc=(1, 1, 0), spill=3.0)
        return pos, typ, h, pbc, g, 90, 2
    if name == "two_free":
        pos, typ, h, pbc = _uniform(500, [10.5, 11.0, 12.0], seed=8, pbc=(0, 1, 0), spill=3.0)
        return pos, typ, h, pbc, g, 90, 2
    if name == "one_eighth":
        pos, typ, h, pbc = _uniform(250, [12.0, 12.5, 13.0], seed=9, corner=0.5)
        return pos, typ, h, pbc, g, 90, 2
    if name == "bins_7":
        pos, typ, h, pbc = _uniform(300, BOX, seed=10)
        return pos, typ, h, pbc, g, 7, 2
    if name == "bins_720":
        pos, typ, h, pbc = _uniform(300, BOX, seed=11)
        return pos, typ, h, pbc, g, 720, 2
    if name == "rmin_2_5":
        pos, typ, h, pbc = _uniform(300, [12.6, 12.9, 13.3], seed=12)
        return pos, typ, h, pbc, global_rows(2.0, 5.0), 90, 2
    if name == "triples":
        pos, typ, h, pbc = _uniform(400, BOX, seed=13)
        return pos, typ, h, pbc, TRIPLE_ROWS, 90, 2
    if name == "absent_itype":
        pos, typ, h, pbc = _uniform(300, BOX, seed=14, typ=np.ones(300))
        return pos, typ, h, pbc, [(0, 1, 1, 0.0, 4.0, 0.0, 4.0), (1, 1, 1, 0.0, 4.0, 0.0, 4.0)], 90, 2
    if name == "rows_32":
        pos, typ, h, pbc = _uniform(300, BOX, seed=15)
        return pos, typ, h, pbc, _rows32(), 720, 2
    raise KeyError(name)


CASES = ["n2", "n3", "n63", "n64", "n65", "n1000", "exactly_2p5_rc", "cells_5_6_9", "triclinic", "one_free", "two_free", "one_eighth",
         "bins_7", "bins_720", "rmin_2_5", "triples", "absent_itype", "rows_32"]
_expected = {}


def _reference(name):
    if name not in _expected:
        pos, typ, h, pbc, rows, nb, T = _case(name)
        counts, amb = expected_counts(pos, typ, h, pbc, rows, nb)
        counts.setflags(write=False)
        _expected[name] = (pos, typ, h, pbc, rows, nb, T, counts, amb)
    return _expected[name]


_engines = {}


def _engine(drv, n):
    if (drv.name, n) not in _engines:
        _engines[(drv.name, n)] = drv.engine(drv.model(NEP), n)
    return _engines[(drv.name, n)]


def _sample_once(drv, pos, typ, h, pbc, rows, nb, T, lds_budget=None, times=1):
    from gpumd_amd.nep import ADF
    a = ADF(_engine(drv, pos.shape[1]), rows, nb, 1, typ, T, lds_budget=lds_budget)
    form = a.form
    for _ in range(times):
        a.sample(drv.dev(pos.reshape(-1)), h, pbc)
    out = a.read()
    a.close()
    return out, form


def lds_fixed(nb):
    cap = (80 * 1024 // 2) // (4 * 32)
    return 4 * cap * 32 + 8 * (nb + 2)


def _check(drv, name):
    pos, typ, h, pbc, rows, nb, T, exp, amb = _reference(name)
    assert not amb.any(), "the case has %d ambiguous triplets: pick another seed" % amb.sum()
    (counts, ns), form = _sample_once(drv, pos, typ, h, pbc, rows, nb, T)
    assert ns == 1
    assert counts.shape == exp.shape and np.array_equal(counts.astype(np.int64), exp), \
        (name, int(np.abs(counts.astype(np.int64) - exp).sum()), int(exp.sum()))
    if pos.shape[1] >= 63:
        assert exp.sum() > 0
    if name == "n2":
        assert not counts.any()
    if name == "absent_itype":
        assert not counts[0].any() and counts[1].any()
    # the counted rule: the table lives in LDS while it fits beside the buffers in half a CU's LDS
    assert form == (1 if lds_fixed(nb) + 4 * exp.size <= 80 * 1024 else 2)
    if name == "rows_32":
        assert form == 2
    (c2, _), _ = _sample_once(drv, pos, typ, h, pbc, rows, nb, T)
    assert np.array_equal(c2, counts)  # bit for bit
    print("\n[%s %s] n=%d triplets=%d form=%d" % (drv.name, name, pos.shape[1], int(exp.sum()), form))


def _lattice():
    g = np.arange(8, dtype=np.float64)
    pos = np.array(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1).copy()
    return pos, np.zeros(512, dtype=np.int32), np.diag([8.0, 8.0, 8.0]).reshape(9), (1, 1, 1)


def _lattice_rules(drv):
    """simple cubic, spacing 1.0, 8^3 atoms"""
    pos, typ, h, pbc = _lattice()
    n = pos.shape[1]
    for nb in (90, 180, 360):  # [0.5, 1.25): six neighbours along the axes, 12 pairs at exactly 90 degrees and 3 at exactly 180
        (counts, _), _ = _sample_once(drv, pos, typ, h, pbc, global_rows(0.5, 1.25), nb, 1)
        exp = np.zeros((1, nb), dtype=np.int64)
        exp[0, nb // 2] = 12 * n
        exp[0, nb - 1] = 3 * n
        assert np.array_equal(counts.astype(np.int64), exp), (nb, np.argwhere(counts.astype(np.int64) != exp))
    # [1, 2): d = 1 is in (closed below), d = 2 is out (open above); d = sqrt 2 and sqrt 3 are in: 6 + 12 + 8 members.  Seven bins:
    # no lattice angle (0, 35.3, 45, 54.7, 60, 70.5, 90, ... 180) lies on an edge k 180 / 7
    ref, amb = expected_counts(pos, typ, h, pbc, global_rows(1.0, 2.0), 7, eps_rel=None)
    assert not amb.any() and ref.sum() == n * 26 * 25 // 2
    (counts, _), _ = _sample_once(drv, pos, typ, h, pbc, global_rows(1.0, 2.0), 7, 1)
    assert np.array_equal(counts.astype(np.int64), ref)
    (counts, _), _ = _sample_once(drv, pos, typ, h, pbc, global_rows(0.5, 1.0), 90, 1)  # d = 1 is out: nothing
    assert not counts.any()


def _accumulation(drv):
    from gpumd_amd.nep import ADF
    n, nb = 300, 90
    a = ADF(_engine(drv, n), (0.0, 4.0), nb, 1)  # the global form needs no types
    c0, s0 = a.read()
    assert not c0.any() and s0 == 0
    total = np.zeros((1, nb), dtype=np.int64)
    for k, L in enumerate((BOX, [11.0, 12.0, 10.2])):
        pos, typ, h, pbc = _uniform(n, L, seed=40 + k)
        exp, amb = expected_counts(pos, typ, h, pbc, global_rows(0.0, 4.0), nb)
        assert not amb.any()
        total += exp
        a.sample(drv.dev(pos.reshape(-1)), h, pbc)
    counts, ns = a.read()
    angle, dens = a.density()
    a.close()
    assert ns == 2 and np.array_equal(counts.astype(np.int64), total)
    assert np.allclose(angle, (np.arange(nb) + 0.5) * 2.0) and np.allclose(dens, total / (total.sum() * 2.0), rtol=1e-14)


def _capacity(drv):
    from gpumd_amd import _capi
    from gpumd_amd.nep import ADF
    cap = int(drv.lib.nepmi_adf_capacity())
    assert cap >= 256 and cap == (80 * 1024 // 2) // (4 * 32)
    rng = np.random.default_rng(77)
    v = rng.normal(size=(3, cap + 2))
    ball = 5.0 + 1.9 * v / np.linalg.norm(v, axis=0) * rng.uniform(0.0, 1.0, cap + 2) ** (1.0 / 3.0)  # diameter 3.8 < rmax = 4
    h, pbc, nb = np.diag([10.5, 10.5, 10.5]).reshape(9), (1, 1, 1), 90
    pos = ball[:, :cap + 1].copy()  # every centre has exactly `cap` members
    exp, amb = expected_counts(pos, np.zeros(cap + 1, dtype=np.int32), h, pbc, global_rows(0.0, 4.0), nb)
    assert not amb.any() and exp.sum() == (cap + 1) * cap * (cap - 1) // 2
    (counts, _), _ = _sample_once(drv, pos, np.zeros(cap + 1, dtype=np.int32), h, pbc, global_rows(0.0, 4.0), nb, 1)
    assert np.array_equal(counts.astype(np.int64), exp)
    pos = ball.copy()  # one atom more: an error code, no fault, nothing counted
    a = ADF(_engine(drv, cap + 2), (0.0, 4.0), nb, 1)
    with pytest.raises(_capi.NepmiError, match="capacity of %d" % cap) as ei:
        a.sample(drv.dev(pos.reshape(-1)), h, pbc)
    assert ei.value.code == -6
    with pytest.raises(_capi.NepmiError) as ei:
        a.read()
    assert ei.value.code == -6
    a.close()


def _refusals(drv):
    from gpumd_amd import _capi
    from gpumd_amd.nep import ADF, AdfRow
    n = 65
    eng = _engine(drv, n)
    typ = np.zeros(n, dtype=np.int32)
    out = C.c_void_p()
    row = (AdfRow * 1)(AdfRow(-1, -1, -1, 0.0, 4.0, 0.0, 4.0))
    st = drv.lib.nepmi_adf_create(eng.handle, n + 1, 90, 1, C.cast(row, C.c_void_p), 1, None, 0, C.byref(out))
    assert st == -4 and b"number of atoms" in drv.lib.nepmi_last_error()
    with pytest.raises(_capi.NepmiError, match="number of bins"):
        ADF(eng, (0.0, 4.0), 0, 1)
    with pytest.raises(_capi.NepmiError, match="number of rows"):
        ADF(eng, [], 90, 1)
    with pytest.raises(_capi.NepmiError, match="number of rows"):
        ADF(eng, global_rows(0.0, 4.0) * 33, 90, 1)
    with pytest.raises(_capi.NepmiError, match="should not be negative"):
        ADF(eng, (-0.5, 4.0), 90, 1)
    with pytest.raises(_capi.NepmiError, match="less than maximum"):
        ADF(eng, (4.0, 4.0), 90, 1)
    with pytest.raises(_capi.NepmiError, match="less than maximum"):
        ADF(eng, [(0, 0, 0, 0.0, 4.0, 3.0, 2.0)], 90, 1, typ, 1)
    with pytest.raises(_capi.NepmiError, match="outside 0"):
        ADF(eng, [(0, 1, 0, 0.0, 4.0, 0.0, 4.0)], 90, 1, typ, 1)
    with pytest.raises(_capi.NepmiError, match="all -1"):
        ADF(eng, [(0, -1, 0, 0.0, 4.0, 0.0, 4.0)], 90, 1, typ, 1)
    with pytest.raises(_capi.NepmiError, match="outside 0"):
        ADF(eng, (0.0, 4.0), 90, 1, np.full(n, 1, dtype=np.int32), 1)
    with pytest.raises(_capi.NepmiError, match="type_of_atom"):
        ADF(eng, [(0, 0, 0, 0.0, 4.0, 0.0, 4.0)], 90, 1, None, 1)
    a = ADF(eng, [(0, 0, 0, 0.0, 2.0, 0.0, 4.0)], 90, 1, typ, 1)  # rc is the largest bound of the rows
    pos, _, h, pbc = _uniform(n, [10.5, 10.5, 9.9], seed=1)
    with pytest.raises(_capi.NepmiError, match="thickness < 2.5 RDF radial cutoffs") as ei:
        a.sample(drv.dev(pos.reshape(-1)), h, pbc)  # rc = 4 > 9.9 / 2.5
    assert ei.value.code == -4
    assert a.read()[1] == 0
    eng.attach(a)
    with pytest.raises(_capi.NepmiError, match="already"):
        eng.attach(a)
    other = drv.engine(eng.model, n)
    with pytest.raises(_capi.NepmiError, match="another engine"):
        other.attach(a)
    eng.detach(a)
    with pytest.raises(_capi.NepmiError, match="not attached"):
        eng.detach(a)
    a2 = ADF(eng, (0.0, 4.0), 90, 2)
    eng.attach(a2)
    a2.close()  # destroying an attached handle detaches it first
    eng.attach(a)
    eng.detach(a)
    a.close()
    other.close()


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    return H.GpuDriver()


@pytest.fixture(scope="module")
def emu():
    return H.EmuDriver()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_counts_on_gpu(gpu, name):
    _check(gpu, name)


@pytest.mark.gpu
def test_lattice_rules_on_gpu(gpu):
    _lattice_rules(gpu)


@pytest.mark.gpu
def test_accumulation_on_gpu(gpu):
    _accumulation(gpu)


@pytest.mark.gpu
def test_capacity_on_gpu(gpu):
    _capacity(gpu)


@pytest.mark.gpu
def test_refusals_on_gpu(gpu):
    _refusals(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rows_32", "triples", "n1000"])
def test_both_forms_agree_on_gpu(gpu, name):
    """the same rows through the LDS tables (for 32 rows at 720 bins with a budget of a whole CU's LDS) and through the global atomics"""
    pos, typ, h, pbc, rows, nb, T, exp, amb = _reference(name)
    (c1, _), f1 = _sample_once(gpu, pos, typ, h, pbc, rows, nb, T, lds_budget=160 * 1024)
    (c2, _), f2 = _sample_once(gpu, pos, typ, h, pbc, rows, nb, T, lds_budget=0)
    assert (f1, f2) == (1, 2)
    assert np.array_equal(c1, c2) and np.array_equal(c1.astype(np.int64), exp)


@pytest.mark.parametrize("name", CASES)
def test_counts_on_emulator(emu, name):
    _check(emu, name)


def test_lattice_rules_on_emulator(emu):
    _lattice_rules(emu)


def test_accumulation_on_emulator(emu):
    _accumulation(emu)


def test_capacity_on_emulator(emu):
    _capacity(emu)


def test_refusals_on_emulator(emu):
    _refusals(emu)
