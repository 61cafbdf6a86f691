"""The orientational-order kernels alone (gpumd_amd/csrc/nep_orient.h) through nepmi_orient_sample on synthetic configurations, in
both tiers: the GPU tier runs the cell binning + the persistent q_lm kernel (+ the average pass) + the columns, the CPU tier (kernel
emulator) the plain body over the same cell list.

Expected values: the definition restated in numpy over ALL pairs, in double (`restate`) -- minimum image through fractional
coordinates; the members of i are the atoms a != i with 0 < d2 < rc^2, mode nnn keeps the k smallest in (d2, index) and none where
fewer than k lie inside the search radius; per member c = z / d, s = rxy / d, e^{i phi} = (x + i y) / rxy (1 where rxy < 1e-15);
Y_lm = sqrt((2l + 1) / 4 pi (l - m)! / (l + m)!) P_l^m e^{i m phi} with the UNNORMALISED Legendre recurrence of the reference
(P_m^m = (2m - 1)!! s^m, no Condon-Shortley sign) and math.factorial -- not the normalised recurrence of the kernel; q_lm the mean
over the members; `average` the mean of q_lm over the atom and its members; q_l, w_l (Clebsch-Gordan coefficients from Racah's sum
in exact rational arithmetic) and what_l as include/nepmi.h states them.

An atom is AMBIGUOUS if a neighbour's d2 lies within a relative 1e-9 of rc^2 or, in mode nnn, if its k-th and (k+1)-th d2 are within
a relative 1e-9; every case asserts first that it has none, nothing is left out.

Tolerances on identical positions: nn equal; |d q_l|, |d w_l| <= 1e-12 (both sides evaluate Y_lm with at most about 3l + 20 roundings
and sum at most 320 terms of magnitude <= sqrt((2l + 1) / 4 pi): |d q| <~ 2 (3l + 340) 2^-53 x 1.41 = 1.2e-13 at l = 12, and q_l is
1-Lipschitz in q up to its prefactor <= 1); |d what_l| <= (f / q_l)^3 1e-12 + 3 |what_l| / q_l 1e-12 with f = sqrt(4 pi / (2l + 1)).
The largest fraction of each bound used is printed.

Shapes: n in {1, 2, 13, 64, 1000} (a wavefront is 64 lanes, a pass of a workgroup four centres; at n = 1000 a centre has about 210
members: several strides of the lanes); a box of exactly 2.5 rc; 5 x 6 x 9 cells; a triclinic box; free directions; all atoms in
one eighth of the box; both modes; degrees [0], [1], [4, 6], [12] and eight degrees with a repeat; every combination of average /
wl / wlhat; lattice shells against the literature's values; the tie rule of mode nnn; the capacity."""
import ctypes as C
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import helpers as H
import test_adf_kernels as AK

NEP = H.golden("PbTe", "nep.txt")
EPS_REL = 1e-9
TOL = 1e-12
RC = 4.0


# ---- the restatement --------------------------------------------------------------------------------------------------------
def clebsch_gordan(l):
    """{(m1, m2): <l m1 l m2 | l m1+m2>} by Racah's sum, the sum in exact rationals"""
    f = math.factorial
    out = {}
    for m1 in range(-l, l + 1):
        for m2 in range(max(-l, -l - m1), min(l, l - m1) + 1):
            m = m1 + m2
            s = Fraction(0)
            for z in range(max(0, -m1, m2), min(l, l - m1, l + m2) + 1):
                s += Fraction((-1) ** z, f(z) * f(l - z) * f(l - m1 - z) * f(l + m2 - z) * f(m1 + z) * f(z - m2))
            pre = Fraction(f(l) ** 3, f(3 * l + 1)) * (f(l + m1) * f(l - m1) * f(l + m2) * f(l - m2) * f(l + m) * f(l - m) * (2 * l + 1))
            out[(m1, m2)] = float(s) * math.sqrt(pre.numerator / pre.denominator)
    return out


def ylm(l, x, y, z, d2):
    """[l + 1, nbonds] complex: Y_lm, m = 0 .. l, of the bonds"""
    d = np.sqrt(d2)
    rxy = np.sqrt(x * x + y * y)
    c, s = z / d, rxy / d
    flat = rxy < 1e-15
    e = np.where(flat, 1.0 + 0.0j, (x + 1j * y) / np.where(flat, 1.0, rxy))
    out = np.zeros((l + 1, len(d2)), dtype=np.complex128)
    em = np.ones(len(d2), dtype=np.complex128)
    for m in range(l + 1):
        p = np.ones(len(d2))
        for i in range(1, m + 1):
            p = p * ((2 * i - 1) * s)
        pm1 = np.zeros(len(d2))
        for i in range(m + 1, l + 1):
            pm2, pm1 = pm1, p
            p = ((2 * i - 1) * c * pm1 - (i + m - 1) * pm2) / (i - m)
        pref = math.sqrt((2 * l + 1) / (4 * math.pi) * (math.factorial(l - m) / math.factorial(l + m)))
        if m > 0:
            em = em * e
        out[m] = pref * p * em
    return out


def bonds(pos, h9, pbc, mode, value, rc_search=6.0, eps_rel=EPS_REL, delta=None):
    """all pairs -> (centre, neighbour, vec [3, nb], d2 [nb], nn [n], ambiguous [n]); pos = [3, n].
    delta (a distance): the ambiguity rule of the run tests instead -- a neighbour within delta of rc, the k-th and (k+1)-th
    distances closer than 2 delta."""
    Hm = np.asarray(h9, dtype=np.float64).reshape(3, 3)
    s = np.linalg.solve(Hm, pos)
    n = pos.shape[1]
    rc = float(value) if mode == "cutoff" else float(rc_search)
    k = 0 if mode == "cutoff" else int(value)
    ci, cj, cv, cd, nn, amb = [], [], [], [], np.zeros(n, dtype=np.int32), np.zeros(n, dtype=bool)
    # large periodic inputs: only the atoms of the slab |ds_0| <= reach / thickness_0 around i can lie within reach of it (a pair's
    # distance is at least |ds_0| thickness_0); the others are left out of the loop below, not out of the definition
    slab = None
    if n > 4096 and pbc[0]:
        s0 = s[0] - np.floor(s[0])
        order = np.argsort(s0, kind="stable")
        s0s = np.concatenate([s0[order] - 1.0, s0[order], s0[order] + 1.0])
        width = (rc * (1.0 + 1e-6) + (0.0 if delta is None else 2.0 * delta)) * np.linalg.norm(np.linalg.inv(Hm)[0])
        slab = (np.concatenate([order, order, order]), s0s, s0, width)
    for i in range(n):
        if slab is not None and slab[3] < 0.45:
            lo, hi = np.searchsorted(slab[1], [slab[2][i] - slab[3], slab[2][i] + slab[3]])
            sub = np.unique(slab[0][lo:hi])
            b = _bonds_of(i, sub, s, Hm, pbc, rc, k, mode, eps_rel, delta)
        else:
            b = _bonds_of(i, None, s, Hm, pbc, rc, k, mode, eps_rel, delta)
        amb[i], mem, dv, d2 = b
        nn[i] = len(mem)
        ci.append(np.full(len(mem), i, dtype=np.int64))
        cj.append(mem.astype(np.int64))
        cv.append(dv)
        cd.append(d2)
    return np.concatenate(ci), np.concatenate(cj), np.concatenate(cv, axis=1), np.concatenate(cd), nn, amb


def _bonds_of(i, sub, s, Hm, pbc, rc, k, mode, eps_rel, delta):
    """the members of atom i among the atoms `sub` (sorted indices, i among them; None: all) -> (ambiguous, members, vec, d2)"""
    ss = s if sub is None else s[:, sub]
    me = i if sub is None else int(np.searchsorted(sub, i))
    ds = ss - s[:, i:i + 1]
    for d in range(3):
        if pbc[d]:
            ds[d] -= np.round(ds[d])
    dv = Hm @ ds
    d2 = (dv * dv).sum(axis=0)
    d2[me] = 0.0
    amb_i = False
    if delta is not None:
        amb_i |= bool((np.abs(np.sqrt(d2) - rc) <= delta).any())
    elif eps_rel is not None:
        amb_i |= bool((np.abs(d2 - rc * rc) <= eps_rel * rc * rc).any())
    mem = np.flatnonzero((d2 > 0.0) & (d2 < rc * rc))
    if mode == "nnn":
        ids = mem if sub is None else sub[mem]
        mem = mem[np.lexsort((ids, d2[mem]))]
        if len(mem) > k:
            a, b = d2[mem[k - 1]], d2[mem[k]]
            if delta is not None:
                amb_i |= bool(np.sqrt(b) - np.sqrt(a) < 2 * delta)
            elif eps_rel is not None:
                amb_i |= bool(b - a <= eps_rel * b)
        mem = mem[:k] if len(mem) >= k else mem[:0]
    return amb_i, (mem if sub is None else sub[mem]), dv[:, mem], d2[mem]


def restate(pos, h9, pbc, mode, value, degrees, average=False, wl=False, wlhat=False, rc_search=6.0, eps_rel=EPS_REL, delta=None,
            pre=None):
    """-> dict(cols [n, ncol], nn [n], amb [n] bool, ql [n, nd], minv [n]: the mean of 1 / d over the members, ci, cj: the bonds);
    pre: what bonds() gave for these positions and this mode"""
    n, nd = pos.shape[1], len(degrees)
    ci, cj, v, d2, nn, amb = pre if pre is not None else bonds(pos, h9, pbc, mode, value, rc_search, eps_rel, delta)
    cnt = np.maximum(nn, 1).astype(np.float64)
    minv = np.bincount(ci, weights=1.0 / np.sqrt(d2), minlength=n) / cnt
    if average:  # an atom is ambiguous as well if a member of it is
        amb = amb | (np.bincount(ci, weights=amb[cj].astype(np.float64), minlength=n) > 0)
    ql, wls, whs = np.zeros((n, nd)), np.zeros((n, nd)), np.zeros((n, nd))
    for il, l in enumerate(degrees):
        Y = ylm(l, v[0], v[1], v[2], d2)
        q = np.zeros((l + 1, n), dtype=np.complex128)
        for m in range(l + 1):
            q[m] = (np.bincount(ci, weights=Y[m].real, minlength=n) + 1j * np.bincount(ci, weights=Y[m].imag, minlength=n)) / cnt
        if average:
            qa = q.copy()
            for m in range(l + 1):
                qa[m] += np.bincount(ci, weights=q[m][cj].real, minlength=n) + 1j * np.bincount(ci, weights=q[m][cj].imag, minlength=n)
            q = qa / (nn + 1.0)
        full = {m: q[m] for m in range(l + 1)}
        for m in range(1, l + 1):
            full[-m] = (-1) ** m * np.conj(q[m])
        f = math.sqrt(4 * math.pi / (2 * l + 1))
        ql[:, il] = f * np.sqrt(sum(np.abs(full[m]) ** 2 for m in range(-l, l + 1)))
        if wl or wlhat:
            w = np.zeros(n)
            for (m1, m2), c in clebsch_gordan(l).items():
                w += c * (full[m1] * full[m2] * np.conj(full[m1 + m2])).real
            w /= math.sqrt(2 * l + 1.0)
            wls[:, il] = w
            ok = ql[:, il] > 1e-15
            whs[ok, il] = w[ok] * (f / ql[ok, il]) ** 3
    cols = [ql] + ([wls] if wl else []) + ([whs] if wlhat else [])
    return dict(cols=np.concatenate(cols, axis=1), nn=nn, amb=amb, ql=ql, minv=minv, ci=ci, cj=cj)


def bounds(ref, degrees, wl, wlhat):
    """[n, ncol] of the tolerances above"""
    ql = ref["ql"]
    n, nd = ql.shape
    out = [np.full((n, nd), TOL)]
    if wl:
        out.append(np.full((n, nd), TOL))
    if wlhat:
        f = np.array([math.sqrt(4 * math.pi / (2 * l + 1)) for l in degrees])[None, :]
        what = ref["cols"][:, -nd:]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            b = np.where(ql > 0, (f / ql) ** 3 * TOL + 3 * np.abs(what) / ql * TOL, 0.0)
        out.append(b)
    return np.concatenate(out, axis=1)


_used = {}


def compare(tag, got_cols, got_nn, ref, degrees, wl, wlhat):
    """nn equal, every column inside its bound; the largest fraction used is printed and kept"""
    assert np.array_equal(got_nn, ref["nn"]), (tag, np.flatnonzero(got_nn != ref["nn"])[:5])
    exp, b = ref["cols"], bounds(ref, degrees, wl, wlhat)
    assert got_cols.shape == exp.shape and np.isfinite(got_cols).all()
    dev = np.abs(got_cols - exp)
    zero = ref["nn"] == 0
    assert not got_cols[zero].any()
    nd = len(degrees)
    names = ["ql"] + (["wl"] if wl else []) + (["wlhat"] if wlhat else [])
    parts = []
    for k, name in enumerate(names):
        d, bb = dev[:, k * nd:(k + 1) * nd], b[:, k * nd:(k + 1) * nd]
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(bb > 0, d / bb, np.where(d > 0, np.inf, 0.0))
        used = float(frac.max()) if frac.size else 0.0
        _used[name] = max(_used.get(name, 0.0), used)
        parts.append("%s %.1e" % (name, used))
        assert (d <= bb).all(), (tag, name, float(d.max()), used)
    print("\n[%s] n=%d bonds=%d  fraction of the bound used: %s" % (tag, len(got_nn), int(ref["nn"].sum()), ", ".join(parts)))


# ---- configurations: name -> (pos [3, n], h9, pbc) -----------------------------------------------------------------------------
def _case(name):
    if name.startswith("n"):
        n = int(name[1:])
        pos, _, h, pbc = AK._uniform(n, AK.BOX, seed=300 + n)
    elif name == "exactly_2p5_rc":
        pos, _, h, pbc = AK._uniform(400, [10.0, 10.0, 10.0], seed=25)
    elif name == "cells_5_6_9":
        pos, _, h, pbc = AK._uniform(700, [2.6 * 4.0, 3.2 * 4.0, 4.7 * 4.0], seed=26)
    elif name == "triclinic":
        h, _, x = H.pbte_supercell((2, 2, 2), rattle=0.05, seed=24)
        pos, pbc = x.reshape(3, -1), (1, 1, 1)
    elif name == "one_free":
        pos, _, h, pbc = AK._uniform(500, [10.5, 11.0, 12.0], seed=27, pbc=(1, 1, 0), spill=3.0)
    elif name == "two_free":
        pos, _, h, pbc = AK._uniform(500, [10.5, 11.0, 12.0], seed=28, pbc=(0, 1, 0), spill=3.0)
    elif name == "one_eighth":
        pos, _, h, pbc = AK._uniform(250, [12.0, 12.5, 13.0], seed=29, corner=0.5)
    elif name == "small":
        pos, _, h, pbc = AK._uniform(300, AK.BOX, seed=30)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(pos), np.asarray(h, dtype=np.float64), pbc


CASES = ["n1", "n2", "n13", "n64", "n1000", "exactly_2p5_rc", "cells_5_6_9", "triclinic", "one_free", "two_free", "one_eighth"]
MODES = {"cutoff": ("cutoff", RC), "nnn": ("nnn", 12)}
DEGREE_SETS = {"l0": [0], "l1": [1], "l4_6": [4, 6], "l12": [12], "eight": [2, 4, 6, 8, 10, 12, 6, 3]}
FLAGS = list(itertools.product((False, True), repeat=3))
_refs = {}


def _reference(name, mode, degrees, average, wl, wlhat):
    key = (name, mode, tuple(degrees), average, wl, wlhat)
    if key not in _refs:
        pos, h, pbc = _case(name)
        m, v = MODES[mode]
        ref = restate(pos, h, pbc, m, v, degrees, average, wl, wlhat, rc_search=RC)
        for a in ref.values():
            a.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


_engines = {}


def _engine(drv, n):
    if (drv.name, n) not in _engines:
        _engines[(drv.name, n)] = drv.engine(drv.model(NEP), n)
    return _engines[(drv.name, n)]


def _sample(drv, pos, h, pbc, mode, value, degrees, average=False, wl=False, wlhat=False, rc_search=RC, times=1):
    from gpumd_amd.nep import OrientOrder
    o = OrientOrder(_engine(drv, pos.shape[1]), mode, value, degrees, average, wl, wlhat, rc_search=rc_search)
    for _ in range(times):
        o.sample(drv.dev(pos.reshape(-1)), h, pbc)
    out = o.read()
    o.close()
    return out


def _check(drv, name, mode, degrees=(4, 6), average=True, wl=True, wlhat=True):
    degrees = list(degrees)
    pos, h, pbc = _case(name)
    ref = _reference(name, mode, degrees, average, wl, wlhat)
    assert not ref["amb"].any(), "the case has %d ambiguous atoms: pick another seed" % ref["amb"].sum()
    m, v = MODES[mode]
    last, total, nn, ns = _sample(drv, pos, h, pbc, m, v, degrees, average, wl, wlhat)
    assert ns == 1 and np.array_equal(last, total)
    compare("%s %s %s %s avg=%d" % (drv.name, name, mode, degrees, average), last, nn, ref, degrees, wl, wlhat)
    if name == "n1":
        assert not last.any() and not nn.any()
    if name == "n1000" and mode == "cutoff":
        assert nn.max() > 192  # more than three strides of the lanes
    if degrees == [0]:
        assert (np.abs(last[nn > 0, 0] - 1.0) <= TOL).all()
    l2, _, n2, _ = _sample(drv, pos, h, pbc, m, v, degrees, average, wl, wlhat)
    assert np.array_equal(l2, last) and np.array_equal(n2, nn)  # the same bits from a second handle


# ---- lattice shells ----------------------------------------------------------------------------------------------------------
def _shell(kind):
    s2, s3 = math.sqrt(2.0), math.sqrt(3.0)
    if kind == "fcc":
        v = [p for p in itertools.product((-1, 0, 1), repeat=3) if sum(abs(c) for c in p) == 2]
        return np.array(v, dtype=np.float64) / s2
    if kind == "hcp":
        z = math.sqrt(2.0 / 3.0)
        plane = [(1, 0, 0), (-1, 0, 0), (.5, s3 / 2, 0), (-.5, s3 / 2, 0), (.5, -s3 / 2, 0), (-.5, -s3 / 2, 0)]
        cap = [(0, 1 / s3, z), (.5, -1 / (2 * s3), z), (-.5, -1 / (2 * s3), z)]
        return np.array(plane + cap + [(x, y, -zz) for x, y, zz in cap], dtype=np.float64)
    if kind == "sc":
        return np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=np.float64)
    if kind == "bcc8":
        return np.array(list(itertools.product((-1, 1), repeat=3)), dtype=np.float64) / s3
    if kind == "bcc14":
        first = np.array(list(itertools.product((-1, 1), repeat=3)), dtype=np.float64) / 2
        return np.concatenate([first, _shell("sc")]) * (2 / s3)  # first shell at 1, second at 2 / sqrt 3
    raise KeyError(kind)


#          q4        q6        what4      what6
LATTICE = {"fcc": (0.190941, 0.574524, -0.159317, -0.013161),
           "hcp": (0.097222, 0.484762, +0.134097, -0.012442),
           "sc": (0.763763, 0.353553, +0.159317, +0.013161),
           "bcc8": (0.509175, 0.628539, -0.159317, +0.013161),
           "bcc14": (0.036370, 0.510688, +0.159317, +0.013161)}
LBOX, LBOND = 20.0, 2.5


def _cluster(kind, rot=None):
    """the centre (atom 0) and its shell, bond length 2.5, in a periodic box of 20"""
    sh = _shell(kind) * LBOND
    if rot is not None:
        sh = sh @ rot.T
    pos = np.concatenate([np.zeros((1, 3)), sh]) + np.array([7.0, 9.0, 8.0])
    return np.ascontiguousarray(pos.T), np.diag([LBOX] * 3).reshape(9), (1, 1, 1)


def _lattices(drv):
    for kind, const in LATTICE.items():
        pos, h, pbc = _cluster(kind)
        k = pos.shape[1] - 1
        for mode, value in (("cutoff", 1.3 * LBOND), ("nnn", k)):
            ref = restate(pos, h, pbc, mode, value, [4, 6], False, True, True, rc_search=1.3 * LBOND, eps_rel=EPS_REL)
            assert not ref["amb"].any() and ref["nn"][0] == k
            last, _, nn, _ = _sample(drv, pos, h, pbc, mode, value, [4, 6], False, True, True, rc_search=1.3 * LBOND)
            compare("%s %s %s" % (drv.name, kind, mode), last, nn, ref, [4, 6], True, True)
            got = (last[0, 0], last[0, 1], last[0, 4], last[0, 5])
            assert np.abs(np.array(got) - np.array(const)).max() <= 5e-7, (kind, mode, got, const)
    # the fcc shell turned by a random orthogonal matrix: the same columns; q5 = 0 there
    rng = np.random.default_rng(12)
    rot, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    degrees = [4, 5, 6]
    pos, h, pbc = _cluster("fcc")
    a, _, nna, _ = _sample(drv, pos, h, pbc, "cutoff", 1.3 * LBOND, degrees, False, True, True)
    pos_r, _, _ = _cluster("fcc", rot)
    ref = restate(pos_r, h, pbc, "cutoff", 1.3 * LBOND, degrees, False, True, True)
    assert not ref["amb"].any()
    b, _, nnb, _ = _sample(drv, pos_r, h, pbc, "cutoff", 1.3 * LBOND, degrees, False, True, True)
    compare("%s fcc turned" % drv.name, b, nnb, ref, degrees, True, True)
    assert np.array_equal(nna, nnb)
    bnd = bounds(ref, degrees, True, True)
    assert (np.abs(a[0] - b[0]) <= bnd[0]).all(), (a[0], b[0])
    for row in (a[0], b[0]):
        assert abs(row[1]) <= TOL and np.isfinite(row[7])  # q5 = 0; what5 is 0 by the q_l <= 1e-15 rule, or inside its (huge) bound
        assert row[7] == 0.0 or abs(row[7]) <= (math.sqrt(4 * math.pi / 11) / row[1]) ** 3 * TOL + 3 * abs(row[7]) / row[1] * TOL


def _tie_rule(drv):
    """mode nnn 2 around atom 0: the nearest at (0, 0, 1), then two atoms at d2 = 4 exactly, one at right angles and one opposite;
    the smaller index of the two is taken.  Dyadic coordinates: every d2 is exact on both sides."""
    h, pbc = np.diag([32.0] * 3).reshape(9), (1, 1, 1)
    c = np.array([8.0, 8.0, 8.0])
    for order, q4_is_one in ((((0, 0, -2), (2, 0, 0)), True), (((2, 0, 0), (0, 0, -2)), False)):
        pos = np.ascontiguousarray((np.array([(0, 0, 0), (0, 0, 1)] + list(order), dtype=np.float64) + c).T)
        ref = restate(pos, h, pbc, "nnn", 2, [4], rc_search=4.0, eps_rel=None)
        last, _, nn, _ = _sample(drv, pos, h, pbc, "nnn", 2, [4], rc_search=4.0)
        compare("%s tie %s" % (drv.name, order), last, nn, ref, [4], False, False)
        assert nn[0] == 2 and (abs(last[0, 0] - 1.0) <= TOL) == q4_is_one, last[0]


def _capacity(drv):
    from gpumd_amd import _capi
    from gpumd_amd.nep import OrientOrder
    cap = int(drv.lib.nepmi_orient_capacity())
    assert cap == 320
    rng = np.random.default_rng(77)
    v = rng.normal(size=(3, cap + 2))
    ball = 5.0 + 1.9 * v / np.linalg.norm(v, axis=0) * rng.uniform(0.0, 1.0, cap + 2) ** (1.0 / 3.0)  # diameter 3.8 < rc = 4
    h, pbc = np.diag([10.5, 10.5, 10.5]).reshape(9), (1, 1, 1)
    pos = np.ascontiguousarray(ball[:, :cap + 1])  # every centre has exactly `cap` members
    for mode, value in (("cutoff", RC), ("nnn", 12)):
        ref = restate(pos, h, pbc, mode, value, [4, 6], False, True, True, rc_search=RC)
        assert not ref["amb"].any() and (ref["nn"] == (cap if mode == "cutoff" else 12)).all()
        last, _, nn, _ = _sample(drv, pos, h, pbc, mode, value, [4, 6], False, True, True)
        compare("%s capacity %s" % (drv.name, mode), last, nn, ref, [4, 6], True, True)
    pos = np.ascontiguousarray(ball)  # one atom more: an error code, no fault, nothing added
    for mode, value in (("cutoff", RC), ("nnn", 12)):
        o = OrientOrder(_engine(drv, cap + 2), mode, value, [4, 6], rc_search=RC)
        with pytest.raises(_capi.NepmiError, match="capacity of %d" % cap) as ei:
            o.sample(drv.dev(pos.reshape(-1)), h, pbc)
        assert ei.value.code == -6
        with pytest.raises(_capi.NepmiError) as ei:
            o.read()
        assert ei.value.code == -6
        o.close()


def _sum_of_three(drv):
    from gpumd_amd.nep import OrientOrder
    n = 300
    o = OrientOrder(_engine(drv, n), "cutoff", RC, [4, 6], True, True, True)
    last, total, nn, ns = o.read()
    assert ns == 0 and not last.any() and not total.any() and not nn.any()
    acc = np.zeros((n, 6))
    for k, L in enumerate((AK.BOX, [11.0, 12.0, 10.2], [10.1, 10.2, 10.3])):
        pos, _, h, pbc = AK._uniform(n, L, seed=60 + k)
        o.sample(drv.dev(np.ascontiguousarray(pos).reshape(-1)), h, pbc)
        last, total, nn, ns = o.read()
        acc = acc + last
        assert ns == k + 1 and np.array_equal(total, acc)  # bit for bit, added in order
    o.close()


def _refusals(drv):
    from gpumd_amd import _capi
    from gpumd_amd.nep import OrientOrder
    n = 65
    eng = _engine(drv, n)
    out = C.c_void_p()
    deg = (C.c_int * 2)(4, 6)

    def create(nn=n, mode=0, rc=4.0, k=0, nd=2, interval=1):
        return drv.lib.nepmi_orient_create(eng.handle, nn, mode, rc, k, deg, nd, 0, 0, 0, interval, C.byref(out))

    assert create(nn=n + 1) == -4 and b"number of atoms" in drv.lib.nepmi_last_error()
    assert create(mode=2) == -4 and b"mode" in drv.lib.nepmi_last_error()
    assert create(interval=0) == -4 and b"interval" in drv.lib.nepmi_last_error()
    for rc in (0.0, -1.0):
        with pytest.raises(_capi.NepmiError, match="cutoff should be a positive"):
            OrientOrder(eng, "cutoff", rc, [4])
    with pytest.raises(_capi.NepmiError, match="nnn should be a positive"):
        OrientOrder(eng, "nnn", 0, [4])
    with pytest.raises(_capi.NepmiError, match="number of degrees"):
        OrientOrder(eng, "cutoff", RC, [])
    with pytest.raises(_capi.NepmiError, match="number of degrees"):
        OrientOrder(eng, "cutoff", RC, [4] * 9)
    with pytest.raises(_capi.NepmiError, match="negative"):
        OrientOrder(eng, "cutoff", RC, [4, -1])
    with pytest.raises(_capi.NepmiError, match="above 12"):
        OrientOrder(eng, "cutoff", RC, [13])
    o = OrientOrder(eng, "nnn", 4, [4, 4, 12], rc_search=RC)  # repeats are allowed
    pos, _, h, pbc = AK._uniform(n, [10.5, 10.5, 9.9], seed=1)
    with pytest.raises(_capi.NepmiError, match="thickness < 2.5") as ei:
        o.sample(drv.dev(np.ascontiguousarray(pos).reshape(-1)), h, pbc)  # rc = 4 > 9.9 / 2.5
    assert ei.value.code == -4
    assert o.read()[3] == 0
    eng.attach(o)
    with pytest.raises(_capi.NepmiError, match="already"):
        eng.attach(o)
    other = drv.engine(eng.model, n)
    with pytest.raises(_capi.NepmiError, match="another engine"):
        other.attach(o)
    eng.detach(o)
    with pytest.raises(_capi.NepmiError, match="not attached"):
        eng.detach(o)
    o2 = OrientOrder(eng, "cutoff", RC, [6], interval=2)
    eng.attach(o2)
    o2.close()  # destroying an attached handle detaches it first
    eng.attach(o)
    eng.detach(o)
    o.close()
    other.close()


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    return H.GpuDriver()


@pytest.fixture(scope="module")
def emu():
    return H.EmuDriver()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", CASES)
def test_columns_on_gpu(gpu, name, mode):
    _check(gpu, name, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("degrees", list(DEGREE_SETS))
def test_degrees_on_gpu(gpu, degrees, mode):
    _check(gpu, "small", mode, DEGREE_SETS[degrees])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("average,wl,wlhat", FLAGS)
def test_flags_on_gpu(gpu, mode, average, wl, wlhat):
    _check(gpu, "n64", mode, (4, 6), average, wl, wlhat)


@pytest.mark.gpu
def test_lattice_shells_on_gpu(gpu):
    _lattices(gpu)


@pytest.mark.gpu
def test_nnn_tie_rule_on_gpu(gpu):
    _tie_rule(gpu)


@pytest.mark.gpu
def test_capacity_on_gpu(gpu):
    _capacity(gpu)


@pytest.mark.gpu
def test_sum_of_three_samples_on_gpu(gpu):
    _sum_of_three(gpu)


@pytest.mark.gpu
def test_refusals_on_gpu(gpu):
    _refusals(gpu)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", CASES)
def test_columns_on_emulator(emu, name, mode):
    _check(emu, name, mode)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("degrees", list(DEGREE_SETS))
def test_degrees_on_emulator(emu, degrees, mode):
    _check(emu, "small", mode, DEGREE_SETS[degrees])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("average,wl,wlhat", FLAGS)
def test_flags_on_emulator(emu, mode, average, wl, wlhat):
    _check(emu, "n64", mode, (4, 6), average, wl, wlhat)


def test_lattice_shells_on_emulator(emu):
    _lattices(emu)


def test_nnn_tie_rule_on_emulator(emu):
    _tie_rule(emu)


def test_capacity_on_emulator(emu):
    _capacity(emu)


def test_sum_of_three_samples_on_emulator(emu):
    _sum_of_three(emu)


def test_refusals_on_emulator(emu):
    _refusals(emu)
