"""`compute_adf` of gpumd-mi against the reference's own program on the same GPU: oracle/_ref/gpumd_ref (see test_ref_md_parity.py)
and gpumd-mi run ref_compare's `pbte_16k` (16,000 atoms, velocities from model.xyz) for 40 steps, once with `compute_adf 4 60 0 4`
and once with `compute_adf 4 60 0 1 1 0 4 0 4 1 0 0 0 4 0 4`: ten blocks each.  The type numbers are the potential's indices
(nep.txt: `nep4 2 Te Pb`, the order test_ref_md_parity_rdf.py counts in): 0-1-1 is Pb-Te-Pb around a Te atom.  Skipped where the
reference binary is not built.  Where oracle/_ref/gpumd_ref_mi is built it runs too and its deviations are printed beside gpumd-mi's.

Header lines: equal as text.  Angles: equal.  Values, per printed number (`%g`, six significant digits), in every block:
    |d| <= 1e-5 max(|a|, |b|) + m x (weight of one triplet in that row),   m = 2 + ceil(8 E),
E the expected number of triplets within the delta band of the bin's two edges, from the reference's own output: the counts of
the adjoining bins per degree x 2 x (180 / pi) delta (1 / d_ia + 1 / d_ib), with both legs at the first-shell distance 3.28 A.
A range bound: the first shell lies at 3.28 A, 0.7 A below the bound at 4 A, but the input is a hot snapshot and atoms of the second
shell (4.64 A, like types: they count in the global form only) dip below 4 A.  Every such seventh neighbour adds six triplets, so
x = (total - 15 x centres) / 6 legs per sample have crossed; spread over the thermal amplitude of 0.1 A at least, x / 0.1 A x 2 delta
of them lie within delta of the bound, with six triplets each, shared among the bins like the counts themselves: that is added to E.
The weight of one triplet is 1 / (total x bin width).  The total is not printed; it is read off the reference's first block, whose
counts are small enough for the six printed digits to show it: the whole number T within 1e-1 of 15 x centres, nearest to it, for
which value x T x width is whole in every bin (asserted: there is one).  Block k takes k x T; what that may be off (the samples'
totals differ by a few 1e-3) is that share of the allowance, which is two triplets at least.
delta = 2e-6 A, the DELTA of test_ref_md_parity_corr.py and _rdf.py (the deviation of the two programs' positions: NOT measured for
this observable before this test ran).  The totals (2.4e5 triplets per sample) stay far below 2^31: the reference's int sums hold.

The test prints the largest deviation in units of one triplet's weight.  On an MI355X: 0 beyond the print quantum in both forms; the
totals read off the first block were 251,130 (global) and 119,455 / 119,445 (the two rows)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

pytestmark = pytest.mark.gpu

STEPS, BINS, INTERVAL = 40, 60, 4
DELTA = 2e-6  # A
FIRST_SHELL = 3.28  # A
LINES = {"global": "compute_adf 4 60 0 4", "triples": "compute_adf 4 60 0 1 1 0 4 0 4 1 0 0 0 4 0 4"}
HEADS = {"global": "#angles total step = %d", "triples": "#angles triples_0-1-1 triples_1-0-0 step = %d"}


def _blocks(path):
    out = []
    for line in open(path).read().splitlines():
        if line.startswith("#"):
            out.append((line, []))
        else:
            out[-1][1].append([float(x) for x in line.split()])
    return [(h, np.array(r)) for h, r in out]


def _total_of_first_block(ref_values, nominal):
    """the row totals the first block's numbers imply: the whole numbers T within 1e-1 of nominal for which value x T x width is
    whole in every bin within the print quantum (the counts are some ten thousand at most there: the quantum is 0.1 of a count)"""
    width = 180.0 / BINS
    out = []
    for m in range(ref_values.shape[1]):
        span = int(round(1e-1 * nominal[m]))
        T = nominal[m] + np.arange(-span, span + 1, dtype=np.float64)
        counts = ref_values[:, m][:, None] * (T * width)[None, :]
        whole = np.round(counts)
        fits = (np.abs(counts - whole) <= 1e-5 * whole + 1e-3).all(axis=0) & (np.abs(whole.sum(axis=0) - T) <= 1.0)
        assert fits.any(), (m, nominal[m], float(np.abs(counts - whole).max(axis=0).min()))
        out.append(T[fits][np.argmin(np.abs(T[fits] - nominal[m]))])
    return np.array(out)


def _allowance(ref_values, total, nominal):
    """ref_values [BINS, M] of one block, total and 15 x centres x samples [M] -> weight [M], m [BINS, M]"""
    width = 180.0 / BINS
    counts = ref_values * (total * width)[None, :]
    crossed = np.maximum(total - nominal, 0.0) / 6.0
    at_bound = crossed / 0.1 * 2.0 * DELTA * 6.0 * counts / total[None, :]
    band = (180.0 / np.pi) * DELTA * (2.0 / FIRST_SHELL)
    pad = np.concatenate([counts[:1], counts, counts[-1:]], axis=0)
    m = np.zeros_like(counts)
    for w in range(BINS):
        e = 0.0
        for lo, hi in ((pad[w], pad[w + 1]), (pad[w + 1], pad[w + 2])):
            e = e + 0.5 * (lo + hi) / width * 2.0 * band
        m[w] = 2 + np.ceil(8.0 * (e + at_bound[w]))
    return 1.0 / (total * width), m


@pytest.mark.parametrize("form", ["global", "triples"])
def test_adf_matches_reference_gpumd(tmp_path, form):
    import ref_compare as R
    from gpumd_amd import structures as S
    if not os.path.exists(R.REF):
        pytest.skip("oracle/_ref/gpumd_ref not built (needs /root/reference at build time)")
    assert os.path.exists(R.MI), "gpumd-mi is not built"
    assert open(os.path.join(R.GOLD, "PbTe", "nep.txt")).readline().split()[1:4] == ["2", "Te", "Pb"]
    exes = [("ref", R.REF), ("mi", R.MI)] + ([("ref_mi", R.REF_MI)] if os.path.exists(R.REF_MI) else [])
    R.FINE = STEPS
    try:
        out = {}
        for tag, exe in exes:
            d = str(tmp_path / tag)
            R.case_inputs("pbte_16k", d)
            run_in = os.path.join(d, "run.in")
            text = open(run_in).read()
            assert "\nrun %d" % STEPS in text
            open(run_in, "w").write(text.replace("\nrun ", "\n%s\nrun " % LINES[form]))
            res, _ = R.run_binary(exe, d, 300.0)
            assert res["rc"] == 0, open(os.path.join(d, "stdout.txt")).read()[-2000:]
            out[tag] = _blocks(os.path.join(d, "adf.out"))
    finally:
        R.FINE = 0
    fr = S.read_xyz_frames(os.path.join(str(tmp_path / "ref"), "model.xyz"))[0]
    species = list(fr["species"])
    n_te, n_pb = species.count("Te"), species.count("Pb")  # (the run leaves the replicated cell in model.xyz)
    assert n_te + n_pb == 16000
    centres = np.array([n_te + n_pb] if form == "global" else [n_te, n_pb], dtype=np.float64)
    ref = out["ref"]
    assert len(ref) == STEPS // INTERVAL
    worst = {t: 0.0 for t, _ in exes if t != "ref"}
    ok = True
    first = _total_of_first_block(ref[0][1][:, 1:], 15.0 * centres)
    print("\n[gpumd_ref, %s] triplets of the first sample per row: %s (15 per centre atom: %s)" % (form, first, 15.0 * centres))
    for k, (head, rows) in enumerate(ref):
        assert head == HEADS[form] % ((k + 1) * INTERVAL - 1), head
        assert rows.shape == (BINS, 1 + len(centres))
        weight, m = _allowance(rows[:, 1:], (k + 1) * first, (k + 1) * 15.0 * centres)
        for tag in worst:
            h1, got = out[tag][k]
            assert h1 == head, (h1, head)
            assert np.array_equal(got[:, 0], rows[:, 0])
            dev = np.abs(got[:, 1:] - rows[:, 1:])
            quantum = 1e-5 * np.maximum(np.abs(got[:, 1:]), np.abs(rows[:, 1:]))
            worst[tag] = max(worst[tag], float((np.maximum(dev - quantum, 0.0) / weight[None, :]).max()))
            if tag == "mi":
                ok = ok and bool((dev <= quantum + m * weight[None, :]).all())
    for tag, w in worst.items():
        print("\n[%s vs gpumd_ref, %s] adf.out, %d blocks: largest (|d| - quantum) in units of one triplet's weight %.3g"
              % (tag, form, len(ref), w))
    assert ok, worst
