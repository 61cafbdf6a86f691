"""The RDF kernels alone (gpumd_amd/csrc/nep_rdf.h) through nepmi_rdf_sample on synthetic configurations, in both tiers: the GPU
tier runs the cell binning + the persistent LDS-histogram pair kernel, the CPU tier (kernel emulator) the plain body over the same
cell list and the same bin rule.

Expected counts: the definition (rdf.cu:97-118) restated in numpy over ALL pairs, in double -- minimum image through fractional
coordinates, a pair counts if 0 < d2 <= rc * rc, in the bin w with (w dr)^2 < d2 <= ((w + 1) dr)^2.  A pair is AMBIGUOUS if its d2
lies within a relative 1e-9 of a squared edge or of rc^2 (the kernel forms the distance from shifted positions, numpy from
fractional differences: they differ by a few 2^-52); every case asserts first that it has none, so the integer counts are equal
EXACTLY.  The edge-rule case has coordinates that are multiples of 2^-4, so every d2 is exact on both sides.

Shapes (the smallest at which the kernel can go wrong): n in {2, 63, 64, 65, 1000} (a wavefront is 64 lanes, a pass 256 centre
atoms); a box of exactly 2.5 rc (five cells: the +-2 reach meets every cell once); 5 x 6 x 9 cells (blocks of 4: partial blocks);
a triclinic box; one and two free directions with atoms outside the box along them; all atoms in one eighth of the box (empty
cells, more than 256 atoms in a block and more than one staging chunk of 512 in a window); 21 and 500 bins; one type, two types
interleaved, two types of which one has no atom, sixteen types at 500 bins (272 KB of table: the form with global atomics)."""
import numpy as np
import pytest

import helpers as H

NEP = H.golden("PbTe", "nep.txt")
EPS_REL = 1e-9


def pair_rows(T):
    return {(a, b): k for k, (a, b) in enumerate((a, b) for a in range(T) for b in range(a, T))}


def expected_counts(pos, typ, h9, pbc, rc, num_bins, T, eps_rel=EPS_REL, eps_abs=None):
    """all pairs -> (counts [P, num_bins], ambiguous [P, num_bins]); pos = [3, n].  eps_abs: a tolerance in DISTANCE instead."""
    Hm = np.asarray(h9, dtype=np.float64).reshape(3, 3)
    s = np.linalg.solve(Hm, pos)
    n = pos.shape[1]
    dr = rc / num_bins
    e = np.arange(num_bins + 1) * dr
    edges2 = e * e
    rows = pair_rows(T)
    P = len(rows)
    counts, amb = np.zeros((P, num_bins), dtype=np.int64), np.zeros((P, num_bins), dtype=np.int64)
    row_of = np.zeros((T, T), dtype=np.int64)
    for (a, b), k in rows.items():
        row_of[a, b] = row_of[b, a] = k
    checks = np.concatenate([edges2, [rc * rc]])
    for i0 in range(0, n, 256):
        i1 = min(n, i0 + 256)
        ds = s[:, None, :] - s[:, i0:i1, None]  # [3, i, j]
        for d in range(3):
            if pbc[d]:
                ds[d] -= np.round(ds[d])
        dv = np.einsum("ab,bij->aij", Hm, ds)
        d2 = (dv * dv).sum(axis=0)
        ii, jj = np.meshgrid(np.arange(i0, i1), np.arange(n), indexing="ij")
        sel = jj > ii
        d2s, ti, tj = d2[sel], typ[ii[sel]], typ[jj[sel]]
        near = d2s <= rc * rc * (1.0 + 1e-6) + (0.0 if eps_abs is None else 4 * rc * eps_abs)
        d2s, ti, tj = d2s[near], ti[near], tj[near]
        row = row_of[ti, tj]
        w = np.searchsorted(edges2, d2s, side="left") - 1
        ok = (d2s <= rc * rc) & (w >= 0) & (w < num_bins)
        np.add.at(counts, (row[ok], w[ok]), 1)
        # ambiguous: near a squared edge (both adjoining bins) or near rc^2 (the last bin)
        if eps_abs is None:
            tol = eps_rel * checks[None, :]
        else:
            tol = 2.0 * np.sqrt(checks)[None, :] * eps_abs + eps_abs * eps_abs
        close = np.abs(d2s[:, None] - checks[None, :]) <= tol
        for k in np.flatnonzero(close.any(axis=1)):
            for c in np.flatnonzero(close[k]):
                for wb in ((c - 1, c) if c <= num_bins else (num_bins - 1,)):
                    if 0 <= wb < num_bins:
                        amb[row[k], wb] += 1
    return counts, amb


def box_volume(h9):
    """the triple product in the order Box::get_volume takes it (src/model/box.cu)"""
    h = [float(v) for v in np.asarray(h9).reshape(9)]
    return abs(h[0] * (h[4] * h[8] - h[5] * h[7]) + h[1] * (h[5] * h[6] - h[3] * h[8]) + h[2] * (h[3] * h[7] - h[4] * h[6]))


# ---- configurations: name -> (pos [3, n], typ, h9, pbc, rc, num_bins, T) ----------------------------------------------------------
def _uniform(n, L, seed, pbc=(1, 1, 1), T=1, typ=None, spill=0.0, corner=1.0):
    rng = np.random.default_rng(seed)
    L = np.asarray(L, dtype=np.float64)
    pos = rng.uniform(0.0, 1.0, (3, n)) * (L * corner)[:, None]
    for d in range(3):
        if not pbc[d] and spill:
            pos[d] = rng.uniform(-spill, L[d] + spill, n)  # a free direction: atoms may lie outside the box
    if typ is None:
        typ = (np.arange(n) * 7 % T).astype(np.int32)  # interleaved membership
    return pos, np.asarray(typ, dtype=np.int32), np.diag(L).reshape(9), pbc


def _case(name):
    rc = 4.0
    if name.startswith("n"):
        n = int(name[1:])
        pos, typ, h, pbc = _uniform(n, [10.4, 10.9, 11.3], seed=100 + n, T=2)
        return pos, typ, h, pbc, rc, 50, 2
    if name == "exactly_2p5_rc":
        pos, typ, h, pbc = _uniform(400, [10.0, 10.0, 10.0], seed=5, T=2)
        return pos, typ, h, pbc, rc, 64, 2
    if name == "cells_5_6_9":
        pos, typ, h, pbc = _uniform(700, [2.6 * rc, 3.2 * rc, 4.7 * rc], seed=6, T=2)
        return pos, typ, h, pbc, rc, 40, 2
    if name == "triclinic":
        h, typ, x = H.pbte_supercell((2, 2, 2), rattle=0.05, seed=4)
        return x.reshape(3, -1), typ, h, (1, 1, 1), 8.0, 100, 2
    if name == "one_free":
        pos, typ, h, pbc = _uniform(500, [10.5, 11.0, 12.0], seed=7, pbc=(1, 1, 0), T=2, spill=3.0)
        return pos, typ, h, pbc, rc, 40, 2
    if name == "two_free":
        pos, typ, h, pbc = _uniform(500, [10.5, 11.0, 12.0], seed=8, pbc=(0, 1, 0), T=2, spill=3.0)
        return pos, typ, h, pbc, rc, 40, 2
    if name == "one_eighth":
        pos, typ, h, pbc = _uniform(1000, [12.0, 12.5, 13.0], seed=9, T=2, corner=0.5)
        return pos, typ, h, pbc, rc, 40, 2
    if name == "bins_21":
        pos, typ, h, pbc = _uniform(300, [10.4, 10.9, 11.3], seed=10, T=2)
        return pos, typ, h, pbc, rc, 21, 2
    if name == "bins_500":
        pos, typ, h, pbc = _uniform(300, [10.4, 10.9, 11.3], seed=11, T=2)
        return pos, typ, h, pbc, rc, 500, 2
    if name == "one_type":
        pos, typ, h, pbc = _uniform(300, [10.4, 10.9, 11.3], seed=12, T=1)
        return pos, typ, h, pbc, rc, 50, 1
    if name == "absent_type":
        pos, typ, h, pbc = _uniform(300, [10.4, 10.9, 11.3], seed=13, typ=np.ones(300))
        return pos, typ, h, pbc, rc, 50, 2
    if name == "sixteen_types":
        pos, typ, h, pbc = _uniform(600, [10.4, 10.9, 11.3], seed=14, T=16)
        return pos, typ, h, pbc, rc, 500, 16
    raise KeyError(name)


CASES = ["n2", "n63", "n64", "n65", "n1000", "exactly_2p5_rc", "cells_5_6_9", "triclinic", "one_free", "two_free", "one_eighth",
         "bins_21", "bins_500", "one_type", "absent_type", "sixteen_types"]
_expected = {}


def _reference(name):
    if name not in _expected:
        pos, typ, h, pbc, rc, nb, T = _case(name)
        counts, amb = expected_counts(pos, typ, h, pbc, rc, nb, T)
        counts.setflags(write=False)
        _expected[name] = (pos, typ, h, pbc, rc, nb, T, counts, amb)
    return _expected[name]


_engines = {}


def _engine(drv, n):
    if (drv.name, n) not in _engines:
        _engines[(drv.name, n)] = drv.engine(drv.model(NEP), n)
    return _engines[(drv.name, n)]


def _sample_once(drv, pos, typ, h, pbc, rc, nb, T, lds_budget=None):
    from gpumd_amd.nep import RDF
    r = RDF(_engine(drv, pos.shape[1]), rc, nb, 1, typ, T, lds_budget=lds_budget)
    form = r.form
    r.sample(drv.dev(pos.reshape(-1)), h, pbc)
    out = r.read()
    r.close()
    return out, form


def _check(drv, name):
    pos, typ, h, pbc, rc, nb, T, exp, amb = _reference(name)
    assert not amb.any(), "the case has %d ambiguous pairs: pick another seed" % amb.sum()
    (counts, vsum, ns), form = _sample_once(drv, pos, typ, h, pbc, rc, nb, T)
    assert ns == 1
    assert counts.shape == exp.shape and np.array_equal(counts.astype(np.int64), exp), \
        (name, int(np.abs(counts.astype(np.int64) - exp).sum()), int(exp.sum()))
    # one product per bin; the determinant here and the engine's are two roundings of the same volume
    assert (np.abs(vsum - counts * box_volume(h)) <= 4 * 2.0 ** -52 * counts * box_volume(h)).all()
    if pos.shape[1] >= 63:
        assert exp.sum() > 0
    # the counted rule: the table lives in LDS while it fits beside the staging buffers in half a CU's LDS
    fixed = 512 * 32 + (512 + 4 + 2 * 512) * 4
    assert form == (1 if fixed + 4 * exp.size <= 80 * 1024 else 2)
    if name == "sixteen_types":
        assert form == 2
    (c2, v2, _), _ = _sample_once(drv, pos, typ, h, pbc, rc, nb, T)
    assert np.array_equal(c2, counts) and np.array_equal(v2, vsum)  # bit for bit
    print("\n[%s %s] n=%d pairs=%d form=%d" % (drv.name, name, pos.shape[1], int(exp.sum()), form))


def _edge_rule(drv):
    """rc = 4, 32 bins: dr = 0.125; coordinates multiples of 2^-4 in a 16 A box (8 cells), every d2 exact"""
    rc, nb, L = 4.0, 32, 16.0
    above = np.nextafter(5.0, np.inf)
    pos = np.array([[1, 1, 1], [2, 1, 1],          # d = 1.0 = 8 dr: bin 7 (closed above), not bin 8
                    [1, 8, 1], [5, 8, 1],          # d = rc: the last bin
                    [1, 1, 8], [above, 1, 8],      # d just above rc: nowhere
                    [8, 8, 8], [8, 8, 8],          # coincident: nowhere
                    [15.5, 14, 14], [0.5, 14, 14]  # d = 1.0 through the periodic boundary, types 1-1
                    ], dtype=np.float64).T.copy()
    typ = np.array([0, 1, 0, 0, 0, 1, 0, 1, 1, 1], dtype=np.int32)
    h = np.diag([L, L, L]).reshape(9)
    exp = np.zeros((3, nb), dtype=np.int64)
    exp[1, 7] = 1   # 0-1
    exp[0, 31] = 1  # 0-0
    exp[2, 7] = 1   # 1-1
    ref, _ = expected_counts(pos, typ, h, (1, 1, 1), rc, nb, 2)
    assert np.array_equal(ref, exp)  # (the numpy restatement agrees with the construction)
    (counts, _, _), _ = _sample_once(drv, pos, typ, h, (1, 1, 1), rc, nb, 2)
    assert np.array_equal(counts.astype(np.int64), exp), np.argwhere(counts.astype(np.int64) != exp)


def _accumulation(drv):
    from gpumd_amd.nep import RDF
    n, rc, nb, T = 300, 4.0, 40, 2
    boxes = ([10.4, 10.9, 11.3], [11.0, 12.0, 10.2], [13.0, 10.1, 10.6])
    r = RDF(_engine(drv, n), rc, nb, 1, (np.arange(n) * 7 % T).astype(np.int32), T)
    c0, v0, s0 = r.read()
    assert not c0.any() and not v0.any() and s0 == 0
    total = np.zeros((3, nb), dtype=np.int64)
    vexp, vmag = np.zeros((3, nb)), np.zeros((3, nb))
    for k, L in enumerate(boxes):
        pos, typ, h, pbc = _uniform(n, L, seed=40 + k, T=T)
        exp, amb = expected_counts(pos, typ, h, pbc, rc, nb, T)
        assert not amb.any()
        total += exp
        vexp += exp * box_volume(h)
        vmag += np.abs(exp * box_volume(h))
        r.sample(drv.dev(pos.reshape(-1)), h, pbc)
    counts, vsum, ns = r.read()
    r.close()
    assert ns == 3 and np.array_equal(counts.astype(np.int64), total)
    assert (np.abs(vsum - vexp) <= 3 * 2.0 ** -52 * vmag).all()


def _refusals(drv):
    from gpumd_amd import _capi
    from gpumd_amd.nep import RDF
    import ctypes as C
    n = 65
    eng = _engine(drv, n)
    typ = np.zeros(n, dtype=np.int32)
    out = C.c_void_p()
    st = drv.lib.nepmi_rdf_create(eng.handle, n + 1, 4.0, 30, 1, np.zeros(n + 1, dtype=np.int32).ctypes.data_as(_capi.c_ip), 1, C.byref(out))
    assert st == -4 and b"number of atoms" in drv.lib.nepmi_last_error()
    with pytest.raises(_capi.NepmiError, match="cutoff should be positive"):
        RDF(eng, 0.0, 30, 1, typ, 1)
    with pytest.raises(_capi.NepmiError, match="number of bins"):
        RDF(eng, 4.0, 0, 1, typ, 1)
    with pytest.raises(_capi.NepmiError, match="outside 0"):
        RDF(eng, 4.0, 30, 1, np.full(n, 1, dtype=np.int32), 1)
    with pytest.raises(_capi.NepmiError, match="outside 0"):
        RDF(eng, 4.0, 30, 1, np.full(n, -1, dtype=np.int32), 1)
    r = RDF(eng, 4.0, 30, 1, typ, 1)
    pos, _, h, pbc = _uniform(n, [10.5, 10.5, 9.9], seed=1)
    with pytest.raises(_capi.NepmiError, match="thickness < 2.5 RDF radial cutoffs") as ei:
        r.sample(drv.dev(pos.reshape(-1)), h, pbc)  # rc = 4 > 9.9 / 2.5
    assert ei.value.code == -4
    assert r.read()[2] == 0
    eng.attach(r)
    with pytest.raises(_capi.NepmiError, match="already"):
        eng.attach(r)
    other = drv.engine(eng.model, n)
    with pytest.raises(_capi.NepmiError, match="another engine"):
        other.attach(r)
    eng.detach(r)
    with pytest.raises(_capi.NepmiError, match="not attached"):
        eng.detach(r)
    r2 = RDF(eng, 4.0, 30, 2, typ, 1)
    eng.attach(r2)
    r2.close()  # destroying an attached handle detaches it first
    eng.attach(r)
    eng.detach(r)
    r.close()
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
def test_edge_rule_on_gpu(gpu):
    _edge_rule(gpu)


@pytest.mark.gpu
def test_accumulation_on_gpu(gpu):
    _accumulation(gpu)


@pytest.mark.gpu
def test_refusals_on_gpu(gpu):
    _refusals(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n1000", "one_eighth", "triclinic"])
def test_both_forms_agree_on_gpu(gpu, name):
    """the same two-type input through the LDS tables and, with a budget of zero bytes, through the global atomics"""
    pos, typ, h, pbc, rc, nb, T, exp, amb = _reference(name)
    (c1, v1, _), f1 = _sample_once(gpu, pos, typ, h, pbc, rc, nb, T)
    (c2, v2, _), f2 = _sample_once(gpu, pos, typ, h, pbc, rc, nb, T, lds_budget=0)
    assert (f1, f2) == (1, 2)
    assert np.array_equal(c1, c2) and np.array_equal(v1, v2) and np.array_equal(c1.astype(np.int64), exp)


@pytest.mark.parametrize("name", CASES)
def test_counts_on_emulator(emu, name):
    _check(emu, name)


def test_edge_rule_on_emulator(emu):
    _edge_rule(emu)


def test_accumulation_on_emulator(emu):
    _accumulation(emu)


def test_refusals_on_emulator(emu):
    _refusals(emu)
