"""The angular-RDF kernels alone (gpumd_amd/csrc/nep_ardf.h) through nepmi_ardf_sample on synthetic configurations, in both tiers:
the GPU tier runs the cell binning + the persistent pair kernel in its two forms (tables in LDS, global atomics), the CPU tier
(kernel emulator) the plain body over the same cell list and the same bin rule.

Expected counts: the definition (include/nepmi.h) restated in numpy over ALL ordered pairs, in double -- minimum image through
fractional coordinates, d = r_j - r_i, theta = arctan2(d_y, d_x); a pair counts if 0 < d2 <= rc^2, in the radial bin w with
lo_w^2 < d2 <= up_w^2 and the smallest azimuth bin t with theta <= up_t, clamped to T - 1 (edges formed as the reference forms
them), the direction -x in bin T - 1.  A pair is AMBIGUOUS if its d2 lies within a relative 1e-9 of a squared r edge or of rc^2,
or its theta within 1e-9 rad of a theta edge or of +-pi (device and host atan2 may differ in the last bits); every case asserts
first that it has none, so the integer counts are equal EXACTLY.  The edge-rule case has coordinates that are multiples of 2^-4.

Shapes: the configurations of test_rdf_kernels.py (n in {2, 63, 64, 65, 1000}, a box of exactly 2.5 rc, 5 x 6 x 9 cells, the
triclinic PbTe cell, one and two free directions with atoms outside the box, all atoms in one eighth of the box, an absent type);
(R, T) in {(21, 21), (50, 36), (500, 24), (30, 1), (1, 30)}; total only, total + (0,0) (0,1) (1,1), (0,1) with (1,0), six pairs at
500 x 64 bins (896 KB of table: the form with global atomics).  Every case whose table fits in LDS runs in both forms."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import test_rdf_kernels as TR

NEP = H.golden("PbTe", "nep.txt")
EPS = 1e-9
P3 = ((0, 0), (0, 1), (1, 1))


def edges(rc, R, T):
    from gpumd_amd.nep import ardf_edges
    r, lo, up, th, th_up = ardf_edges(rc, R, T)
    return lo, up, th_up


def expected_ardf(pos, typ, h9, pbc, rc, R, T, pairs, eps=EPS):
    """all ordered pairs -> (counts [C, R, T] int64, number of ambiguous pairs); pos = [3, n]"""
    Hm = np.asarray(h9, dtype=np.float64).reshape(3, 3)
    s = np.linalg.solve(Hm, pos)
    n = pos.shape[1]
    lo, up, th_up = edges(rc, R, T)
    lo2, up2 = lo * lo, up * up
    checks = np.concatenate([lo2, up2, [rc * rc]])
    counts = np.zeros((1 + len(pairs), R, T), dtype=np.int64)
    amb = 0
    for i0 in range(0, n, 256):
        i1 = min(n, i0 + 256)
        ds = s[:, None, :] - s[:, i0:i1, None]  # [3, i, j] = s_j - s_i
        for d in range(3):
            if pbc[d]:
                ds[d] -= np.round(ds[d])
        dv = np.einsum("ab,bij->aij", Hm, ds)
        d2 = (dv * dv).sum(axis=0)
        ii, jj = np.meshgrid(np.arange(i0, i1), np.arange(n), indexing="ij")
        sel = (jj != ii) & (d2 <= rc * rc * (1.0 + 1e-6))
        d2s, dx, dy, ti, tj = d2[sel], dv[0][sel], dv[1][sel], typ[ii[sel]], typ[jj[sel]]
        theta = np.arctan2(dy, dx)
        w = np.searchsorted(up2, d2s, side="left")
        t = np.minimum(np.searchsorted(th_up, theta, side="left"), T - 1)
        t[(dy == 0.0) & (dx < 0.0)] = T - 1
        ok = (d2s <= rc * rc) & (d2s > lo2[0]) & (w < R)
        w, t = np.minimum(w, R - 1), t
        np.add.at(counts[0], (w[ok], t[ok]), 1)
        for c, (a, b) in enumerate(pairs):
            m = ok & (ti == a) & (tj == b)
            np.add.at(counts[c + 1], (w[m], t[m]), 1)
        near_r = (np.abs(d2s[:, None] - checks[None, :]) <= eps * checks[None, :]).any(axis=1)
        near_t = (np.abs(theta[:, None] - th_up[None, :]) <= eps).any(axis=1) | (np.abs(theta) >= np.pi - eps)
        exact_x = (dy == 0.0) & (dx != 0.0)  # (+-x on exact coordinates is the edge-rule case's subject, not an ambiguity)
        amb += int((near_r | (near_t & ~exact_x & (T > 1))).sum())
    return counts, amb


# name -> (configuration of test_rdf_kernels, R, T, pairs)
CASES = {
    "n2": ("n2", 50, 36, P3), "n63": ("n63", 50, 36, P3), "n64": ("n64", 50, 36, P3), "n65": ("n65", 50, 36, P3),
    "n1000": ("n1000", 50, 36, P3), "exactly_2p5_rc": ("exactly_2p5_rc", 21, 21, P3), "cells_5_6_9": ("cells_5_6_9", 40, 24, P3),
    "triclinic": ("triclinic", 40, 24, P3), "one_free": ("one_free", 30, 24, P3), "two_free": ("two_free", 30, 24, P3),
    "one_eighth": ("one_eighth", 40, 36, P3), "bins_500x24": ("bins_500", 500, 24, ()), "bins_30x1": ("bins_21", 30, 1, P3),
    "bins_1x30": ("bins_21", 1, 30, P3), "total_only": ("one_type", 50, 36, ()), "absent_type": ("absent_type", 50, 36, P3),
    "swapped": ("n1000", 50, 24, ((0, 1), (1, 0))),
    "six_pairs": ("sixteen_types", 500, 64, ((0, 0), (0, 1), (1, 0), (1, 1), (2, 3), (15, 15))),
}
_expected = {}


def _reference(name):
    if name not in _expected:
        cfg, R, T, pairs = CASES[name]
        pos, typ, h, pbc, rc, _, nt = TR._case(cfg)
        counts, amb = expected_ardf(pos, typ, h, pbc, rc, R, T, pairs)
        counts.setflags(write=False)
        _expected[name] = (pos, typ, h, pbc, rc, R, T, pairs, nt, counts, amb)
    return _expected[name]


_engines = {}


def _engine(drv, n):
    if (drv.name, n) not in _engines:
        _engines[(drv.name, n)] = drv.engine(drv.model(NEP), n)
    return _engines[(drv.name, n)]


def _sample_once(drv, pos, typ, h, pbc, rc, R, T, pairs, nt, lds_budget=None):
    from gpumd_amd.nep import ARDF
    r = ARDF(_engine(drv, pos.shape[1]), rc, R, T, 1, typ, nt, pairs)
    if lds_budget is not None:
        r.set_lds_budget(lds_budget)
    form = r.form
    r.sample(drv.dev(pos.reshape(-1)), h, pbc)
    out = r.read()
    r.close()
    return out, form


def _rdf_counts(drv, pos, typ, h, pbc, rc, R, nt):
    from gpumd_amd.nep import RDF
    r = RDF(_engine(drv, pos.shape[1]), rc, R, 1, typ, nt)
    r.sample(drv.dev(pos.reshape(-1)), h, pbc)
    counts = r.read()[0].astype(np.int64)
    r.close()
    return counts


def _check(drv, name):
    pos, typ, h, pbc, rc, R, T, pairs, nt, exp, amb = _reference(name)
    assert amb == 0, "the case has %d ambiguous pairs: pick another seed" % amb
    (counts, vsum, ns), form = _sample_once(drv, pos, typ, h, pbc, rc, R, T, pairs, nt)
    got = counts.astype(np.int64)
    assert ns == 1
    assert got.shape == exp.shape and np.array_equal(got, exp), (name, int(np.abs(got - exp).sum()), int(exp.sum()))
    vol = TR.box_volume(h)
    assert (np.abs(vsum - counts * vol) <= 4 * 2.0 ** -52 * counts * vol).all()
    if pos.shape[1] >= 63:
        assert exp[0].sum() > 0
    # the counted rule: the table lives in LDS while it fits beside the staging buffers in half a CU's LDS
    fixed = 512 * 32 + (512 + 4 + 2 * 512) * 4
    assert form == (1 if fixed + 4 * exp.size <= 80 * 1024 else 2)
    if name == "six_pairs":
        assert form == 2
    if form == 1:  # the other form on the same input
        (c2, v2, _), f2 = _sample_once(drv, pos, typ, h, pbc, rc, R, T, pairs, nt, lds_budget=0)
        assert f2 == 2 and np.array_equal(c2, counts) and np.array_equal(v2, vsum)
    # marginals: summed over theta the table is the RDF of the kernel that already stands (same bins where no pair is ambiguous)
    rdf = _rdf_counts(drv, pos, typ, h, pbc, rc, R, nt)
    rows = TR.pair_rows(nt)
    marg = got.sum(axis=2)
    assert np.array_equal(marg[0], 2 * rdf.sum(axis=0))
    for c, (a, b) in enumerate(pairs):
        row = rdf[rows[(min(a, b), max(a, b))]]
        assert np.array_equal(marg[c + 1], 2 * row if a == b else row), (name, a, b)
    if name == "swapped":  # (0,1) and (1,0): each other's half-turn
        assert np.array_equal(got[2], np.roll(got[1], T // 2, axis=1))
    print("\n[%s %s] n=%d ordered pairs=%d form=%d" % (drv.name, name, pos.shape[1], int(exp[0].sum()), form))


def _edge_rule(drv, T):
    """rc = 4, 32 radial bins: dr = 0.125; coordinates multiples of 2^-4 in a 16 A box, free along y, every d2 exact"""
    rc, R, L = 4.0, 32, 16.0
    above = np.nextafter(5.0, np.inf)
    pos = np.array([[1, 1, 1], [2, 1, 1],             # d = 1.0 = 8 dr along +x: radial bin 7 (closed above); reverse: -x
                    [1, 8, 1], [5, 8, 1],             # d = rc along +x: the last radial bin
                    [1, 1, 8], [above, 1, 8],         # d just above rc: nowhere
                    [8, 8, 8], [8, 8, 8],             # coincident: nowhere
                    [15.5, 14, 14], [0.5, 14, 14],    # d = 1.0 through the periodic boundary, types 1-1
                    [3, -0.0, 12], [2, 0.0, 12],      # -x from the first to the second, d_y = +0 - (-0)
                    [13, 0.0, 5], [12, -0.0, 5],      # -x from the first to the second, d_y = (-0) - (+0) = -0
                    [9, 3, 3], [9, 3, 4.5]            # along z: d_x = d_y = 0, theta = 0 both ways
                    ], dtype=np.float64).T.copy()
    typ = np.array([0, 1, 0, 0, 0, 1, 0, 1, 1, 1, 0, 0, 0, 0, 1, 1], dtype=np.int32)
    h = np.diag([L, L, L]).reshape(9)
    pbc = (1, 0, 1)
    pairs = ((0, 1), (0, 0), (1, 1))
    lo, up, th_up = edges(rc, R, T)
    zero = min(int(np.searchsorted(th_up, 0.0, side="left")), T - 1)  # the bin of theta = 0 by the rule
    exp = np.zeros((4, R, T), dtype=np.int64)
    for w, c, n_fwd in ((7, 1, 1), (31, 2, 2), (7, 3, 2), (7, 2, 2), (7, 2, 2)):  # (radial bin, column, counts of the column a direction)
        exp[0, w, zero] += 1
        exp[0, w, T - 1] += 1
        if c == 1:
            exp[1, w, zero] += 1  # 0 -> 1 is +x
        else:
            exp[c, w, zero] += 1
            exp[c, w, T - 1] += 1
    exp[0, 11, zero] += 2  # along z, d = 1.5 = 12 dr: bin 11, theta = 0 both ways
    exp[3, 11, zero] += 2
    ref, _ = expected_ardf(pos, typ, h, pbc, rc, R, T, pairs)
    assert np.array_equal(ref, exp), np.argwhere(ref != exp)  # (the numpy restatement agrees with the construction)
    (counts, _, _), _ = _sample_once(drv, pos, typ, h, pbc, rc, R, T, pairs, 2)
    assert np.array_equal(counts.astype(np.int64), exp), np.argwhere(counts.astype(np.int64) != exp)


def _symmetry(drv):
    """a quarter turn about z, (x, y) -> (-y, x), exact: with 24 azimuth bins every count moves by 6 bins"""
    n, rc, R, T, L = 400, 4.0, 40, 24, 11.0
    rng = np.random.default_rng(21)
    pos = rng.uniform(-0.5 * L, 0.5 * L, (3, n))
    typ = (np.arange(n) * 7 % 2).astype(np.int32)
    h = np.diag([L, L, L]).reshape(9)
    rot = np.stack([-pos[1], pos[0], pos[2]])
    tabs = []
    for p in (pos, rot):
        exp, amb = expected_ardf(p, typ, h, (1, 1, 1), rc, R, T, P3)
        assert amb == 0
        (counts, _, _), _ = _sample_once(drv, p, typ, h, (1, 1, 1), rc, R, T, P3, 2)
        assert np.array_equal(counts.astype(np.int64), exp)
        tabs.append(counts)
    assert tabs[0].sum() > 0 and np.array_equal(tabs[1], np.roll(tabs[0], 6, axis=2))


def _accumulation(drv):
    from gpumd_amd.nep import ARDF
    n, rc, R, T = 300, 4.0, 40, 24
    boxes = ([10.4, 10.9, 11.3], [11.0, 12.0, 10.2], [13.0, 10.1, 10.6])
    typ = (np.arange(n) * 7 % 2).astype(np.int32)
    r = ARDF(_engine(drv, n), rc, R, T, 1, typ, 2, P3)
    c0, v0, s0 = r.read()
    assert not c0.any() and not v0.any() and s0 == 0
    total = np.zeros((4, R, T), dtype=np.int64)
    vexp = np.zeros((4, R, T))
    for k, L in enumerate(boxes):
        pos, _, h, pbc = TR._uniform(n, L, seed=40 + k, T=2)
        exp, amb = expected_ardf(pos, typ, h, pbc, rc, R, T, P3)
        assert amb == 0
        total += exp
        vexp += exp * TR.box_volume(h)
        r.sample(drv.dev(pos.reshape(-1)), h, pbc)
    counts, vsum, ns = r.read()
    r.close()
    assert ns == 3 and np.array_equal(counts.astype(np.int64), total)
    assert (np.abs(vsum - vexp) <= 3 * 2.0 ** -52 * vexp).all()


def _two_handles(drv):
    from gpumd_amd.nep import ARDF
    pos, typ, h, pbc, rc, R, T, pairs, nt, exp, amb = _reference("cells_5_6_9")
    eng = _engine(drv, pos.shape[1])
    a, b = ARDF(eng, rc, R, T, 1, typ, nt, pairs), ARDF(eng, rc, R, T, 1, typ, nt, pairs)
    x = drv.dev(pos.reshape(-1))
    a.sample(x, h, pbc)
    b.sample(x, h, pbc)
    (ca, va, _), (cb, vb, _) = a.read(), b.read()
    a.close()
    b.close()
    assert np.array_equal(ca, cb) and np.array_equal(va, vb) and np.array_equal(ca.astype(np.int64), exp)


def _refusals(drv):
    from gpumd_amd import _capi
    from gpumd_amd.nep import ARDF
    n = 65
    eng = _engine(drv, n)
    typ = np.zeros(n, dtype=np.int32)
    out = C.c_void_p()
    ip = _capi.c_ip
    st = drv.lib.nepmi_ardf_create(eng.handle, n + 1, 4.0, 30, 24, 1, None, 1, 0, None, C.byref(out))
    assert st == -4 and b"number of atoms" in drv.lib.nepmi_last_error()
    seven = np.zeros(14, dtype=np.int32)
    for npairs in (7, -1):
        st = drv.lib.nepmi_ardf_create(eng.handle, n, 4.0, 30, 24, 1, typ.ctypes.data_as(ip), 1, npairs, seven.ctypes.data_as(ip), C.byref(out))
        assert st == -4 and b"type pairs should be 0 .. 6" in drv.lib.nepmi_last_error()
    with pytest.raises(_capi.NepmiError, match="cutoff should be positive"):
        ARDF(eng, 0.0, 30, 24, 1)
    for R in (0, 501):
        with pytest.raises(_capi.NepmiError, match="radial bins"):
            ARDF(eng, 4.0, R, 24, 1)
    for T in (0, 1025):
        with pytest.raises(_capi.NepmiError, match="theta bins"):
            ARDF(eng, 4.0, 30, T, 1)
    with pytest.raises(_capi.NepmiError, match="outside 0"):
        ARDF(eng, 4.0, 30, 24, 1, np.full(n, 1, dtype=np.int32), 1)
    with pytest.raises(_capi.NepmiError, match="outside 0"):
        ARDF(eng, 4.0, 30, 24, 1, np.full(n, -1, dtype=np.int32), 1)
    with pytest.raises(_capi.NepmiError, match="type pair holds a type outside 0"):
        ARDF(eng, 4.0, 30, 24, 1, typ, 1, ((0, 1),))  # a type index equal to num_types
    with pytest.raises(_capi.NepmiError, match="type pair holds a type outside 0"):
        ARDF(eng, 4.0, 30, 24, 1, typ, 1, ((-1, 0),))
    with pytest.raises(_capi.NepmiError, match="need pair_types and type_of_atom"):
        ARDF(eng, 4.0, 30, 24, 1, None, 1, ((0, 0),))
    r = ARDF(eng, 4.0, 30, 24, 1)  # no pairs: type_of_atom may be absent
    pos, _, h, pbc = TR._uniform(n, [10.5, 10.5, 9.9], seed=1)
    with pytest.raises(_capi.NepmiError, match="thickness < 2.5 RDF radial cutoffs") as ei:
        r.sample(drv.dev(pos.reshape(-1)), h, pbc)  # rc = 4 > 9.9 / 2.5
    assert ei.value.code == -4
    assert r.read()[2] == 0
    r.sample(drv.dev(pos.reshape(-1)), h, (1, 1, 0))  # ... in a PERIODIC direction only
    assert r.read()[2] == 1
    r.attach()
    with pytest.raises(_capi.NepmiError, match="already"):
        eng.attach(r)
    other = drv.engine(eng.model, n)
    with pytest.raises(_capi.NepmiError, match="another engine"):
        other.attach(r)
    r.detach()
    with pytest.raises(_capi.NepmiError, match="not attached"):
        eng.detach(r)
    r2 = ARDF(eng, 4.0, 30, 24, 2)
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
@pytest.mark.parametrize("name", list(CASES))
def test_counts_on_gpu(gpu, name):
    _check(gpu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [21, 24, 36])
def test_edge_rule_on_gpu(gpu, T):
    _edge_rule(gpu, T)


@pytest.mark.gpu
def test_symmetry_on_gpu(gpu):
    _symmetry(gpu)


@pytest.mark.gpu
def test_accumulation_on_gpu(gpu):
    _accumulation(gpu)


@pytest.mark.gpu
def test_two_handles_on_gpu(gpu):
    _two_handles(gpu)


@pytest.mark.gpu
def test_refusals_on_gpu(gpu):
    _refusals(gpu)


@pytest.mark.parametrize("name", list(CASES))
def test_counts_on_emulator(emu, name):
    _check(emu, name)


@pytest.mark.parametrize("T", [21, 24, 36])
def test_edge_rule_on_emulator(emu, T):
    _edge_rule(emu, T)


def test_symmetry_on_emulator(emu):
    _symmetry(emu)


def test_accumulation_on_emulator(emu):
    _accumulation(emu)


def test_two_handles_on_emulator(emu):
    _two_handles(emu)


def test_refusals_on_emulator(emu):
    _refusals(emu)
