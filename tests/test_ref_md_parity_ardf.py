"""`compute_angular_rdf` of gpumd-mi against the reference's own program on the same GPU: oracle/_ref/gpumd_ref (see
test_ref_md_parity.py) and gpumd-mi run ref_compare's `pbte_16k` (16,000 atoms, velocities from model.xyz) for 40 steps with
`compute_angular_rdf 8 40 24 4 atom 0 0 atom 0 1 atom 1 1` (and `compute_rdf 8 40 4` beside it): ten samples.  Skipped where the
reference binary is not built.  Where oracle/_ref/gpumd_ref_mi is built it runs too and its deviations are printed beside gpumd-mi's.

The header line of angular_rdf.out: equal as text.  Values, per printed number (`%.5f`):
    |d| <= 1e-5 + m x (weight of one pair in that bin and column),   m = 2 + ceil(8 E),
E the expected number of pairs, over all samples, within delta of the bin's two r edges or within delta / r_xy of its two theta
edges, estimated from the reference's own values: counts c = g / weight; an r edge: the mean count of the two adjoining r bins
/ dr x 2 delta; a theta edge: the counts of the two adjoining theta bins x (pi / 2) delta / (r_w D) (the mean of 1 / r_xy over
directions is (pi / 2) / r).  A pair's weight: total V / (N^2 bv S), (a, a) V / (N_a^2 bv S), (a, b) V / (N_a N_b bv S),
bv = D / (2 pi) * 4 pi / 3 (up^3 - lo^3), S = steps / interval.
delta = 2e-6 A is the figure four earlier parity tests used; it has NOT been measured for this observable.  The test prints the
largest deviation in units of one pair's weight and the share of the allowance used.

The reference tests a pair against every bin and so drops or doubles pairs at its own bin edges.  They are counted from the
reference's files -- its total column summed over theta, as ordered pairs per r bin, against the same number from its rdf.out
(resolution of the printed rdf.out: about two pairs a bin) -- and reported, not absorbed into m."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

pytestmark = pytest.mark.gpu

STEPS, RC, R, T, INTERVAL = 40, 8.0, 40, 24, 4
PAIRS = ((0, 0), (0, 1), (1, 1))
DELTA = 2e-6  # A
KEYWORD = "compute_angular_rdf %g %d %d %d" % (RC, R, T, INTERVAL) + "".join(" atom %d %d" % p for p in PAIRS)


def _block(path):
    lines = open(path).read().splitlines()
    return lines[0], np.array([[float(x) for x in r.split()] for r in lines[1:]])


def _weights(n_of_type, volume):
    """-> weight of one pair [C, R, 1]"""
    from gpumd_amd.nep import ardf_edges
    samples = STEPS // INTERVAL
    r, lo, up, th, _ = ardf_edges(RC, R, T)
    bv = (1.0 / T) * 4.0 / 3.0 * np.pi * (up ** 3 - lo ** 3)
    N = float(sum(n_of_type))
    norm = [N * N] + [float(n_of_type[a]) * float(n_of_type[b]) for a, b in PAIRS]
    return np.stack([volume / (w * bv * samples) for w in norm])[:, :, None], r


def _allowance(g_ref, weight, r):
    """m [C, R, T] from the reference's own values"""
    dr, D = RC / R, 2.0 * np.pi / T
    c = g_ref / weight  # counts over all samples
    cp = np.concatenate([c[:, :1], c, c[:, -1:]], axis=1)
    e_r = (0.5 * (cp[:, :-2] + cp[:, 1:-1]) + 0.5 * (cp[:, 1:-1] + cp[:, 2:])) / dr * 2.0 * DELTA
    e_t = ((c + np.roll(c, 1, axis=2)) + (c + np.roll(c, -1, axis=2))) * (np.pi / 2.0) * DELTA / (r[None, :, None] * D)
    return 2 + np.ceil(8.0 * (e_r + e_t))


def test_angular_rdf_matches_reference_gpumd(tmp_path):
    import ref_compare as RCMP
    from gpumd_amd import structures as S
    if not os.path.exists(RCMP.REF):
        pytest.skip("oracle/_ref/gpumd_ref not built (needs /root/reference at build time)")
    assert os.path.exists(RCMP.MI), "gpumd-mi is not built"
    exes = [("ref", RCMP.REF), ("mi", RCMP.MI)] + ([("ref_mi", RCMP.REF_MI)] if os.path.exists(RCMP.REF_MI) else [])
    RCMP.FINE = STEPS
    try:
        out, rdf = {}, {}
        for tag, exe in exes:
            d = str(tmp_path / tag)
            RCMP.case_inputs("pbte_16k", d)
            run_in = os.path.join(d, "run.in")
            text = open(run_in).read()
            assert "\nrun %d" % STEPS in text
            open(run_in, "w").write(text.replace("\nrun ", "\n%s\ncompute_rdf %g %d %d\nrun " % (KEYWORD, RC, R, INTERVAL)))
            res, _ = RCMP.run_binary(exe, d, 300.0)
            assert res["rc"] == 0, open(os.path.join(d, "stdout.txt")).read()[-2000:]
            out[tag] = _block(os.path.join(d, "angular_rdf.out"))
            rdf[tag] = _block(os.path.join(d, "rdf.out"))
    finally:
        RCMP.FINE = 0
    fr = S.read_xyz_frames(os.path.join(str(tmp_path / "ref"), "model.xyz"))[0]
    species = list(fr["species"])
    n_of_type = [species.count("Te"), species.count("Pb")]  # the potential's order
    volume = abs(np.linalg.det(fr["lattice"]))
    head, ref = out["ref"]
    C = 1 + len(PAIRS)
    assert head == "#radius theta total type_0_0 type_0_1 type_1_1", head
    assert ref.shape == (R * T, 2 + C) and ref[:, 2].max() > 1.0
    weight, r = _weights(n_of_type, volume)
    g_ref = ref[:, 2:].T.reshape(C, R, T)
    m = _allowance(g_ref, weight, r)
    # the reference's own dropped / doubled pairs: ordered pairs per r bin from its total column against its rdf.out
    samples = STEPS // INTERVAL
    N = float(sum(n_of_type))
    dr = RC / R
    dV = 4.0 * np.pi * r * r * dr
    for tag in ("ref", "mi"):
        n_ardf = (out[tag][1][:, 2].reshape(R, T) / weight[0]).sum(axis=1)
        n_rdf = rdf[tag][1][:, 1] * N * N * dV * samples / volume
        print("\n[%s] ordered pairs, total column summed over theta minus rdf.out's: net %.1f, sum of |differences| per r bin %.1f "
              "(of %.0f pairs; a printed rdf.out resolves about %.1f pairs a bin)"
              % (tag, (n_ardf - n_rdf).sum(), np.abs(n_ardf - n_rdf).sum(), n_rdf.sum(), 1e-5 * N * N * dV.mean() * samples / volume))
    worst = {}
    for tag in [t for t, _ in exes if t != "ref"]:
        h1, rows = out[tag]
        assert h1 == head, (h1, head)
        assert np.array_equal(rows[:, :2], ref[:, :2])
        dev = np.abs(rows[:, 2:] - ref[:, 2:]).T.reshape(C, R, T)
        worst[tag] = float((dev / weight).max())
        print("\n[%s vs gpumd_ref] angular_rdf.out: largest |d| %.2e; in units of one pair's weight %.3g (allowance m: %d .. %d); "
              "largest share of the allowance used, (|d| - 1e-5) / (m weight): %.3g"
              % (tag, dev.max(), worst[tag], int(m.min()), int(m.max()), float(((dev - 1e-5) / (m * weight)).max())))
    dev = np.abs(out["mi"][1][:, 2:] - ref[:, 2:]).T.reshape(C, R, T)
    assert (dev <= 1e-5 + m * weight).all(), worst
