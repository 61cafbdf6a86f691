"""`compute_adf` in gpumd-mi (gpumd_amd/host/run.cpp), both forms of the keyword: the run dumps its frames with `dump_xyz` at the
sample interval and every block of adf.out is recomputed from them in numpy (test_adf_kernels.expected_counts: all triplets, minimum
image, the mask rule, definition D), then the output half of ADF::process: one block per sample with the CUMULATIVE counts, the
header `#angles total step = <0-based step>` or `#angles triples_i-j-k ... step = <step>`, the bin centres, every row divided by
its own total x the bin width.

Tolerance.  dump_xyz prints nine significant digits: coordinates of 10 .. 100 A are rounded by at most delta = 5e-8 A.  A triplet is
ambiguous if a leg lies within 2 sqrt(3) delta of a bound or its angle within (180 / pi) 2 sqrt(3) delta (1 / d_ia + 1 / d_ib) of a
bin edge; asserted first: they are at most 1e-3 of the counted triplets.  Every printed number within the `%g` rounding (six
significant digits: a relative 5e-6, asked as 1e-5) plus the ambiguous triplets' weight in that bin and row.  Headers as text.

CPU tier: the host linked against the kernel emulator (tests/emu/gpumd-mi-emu), the 250-atom PbTe cell replicated 2 x 2 x 2 (38 A
thick); one GPU case with the product binary on 3 x 3 x 3.  Input errors through --check-input."""
import os
import socket
import subprocess

import numpy as np
import pytest

import helpers as H
import test_adf_kernels as AK
import test_host_rdf as HR

EMU, EXE, HEAD, SYMBOLS = HR.EMU, HR.EXE, HR.HEAD, HR.SYMBOLS
DELTA = 2.0 * np.sqrt(3.0) * 5e-8
BINS = 90
GLOBAL_LINE, GLOBAL_ROWS = "compute_adf 5 90 0 4", AK.global_rows(0.0, 4.0)
TRIPLE_LINE = "compute_adf 5 90 0 1 1 2 5 2 5 1 0 0 2 5 2 5 0 0 1 2 5 2 5"
TRIPLE_ROWS = [(0, 1, 1, 2.0, 5.0, 2.0, 5.0), (1, 0, 0, 2.0, 5.0, 2.0, 5.0), (0, 0, 1, 2.0, 5.0, 2.0, 5.0)]


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(H.ROOT, "tests", "emu"), "all"], check=True)


def _header(rows, step):
    if rows is GLOBAL_ROWS:
        return "#angles total step = %d" % step
    return "#angles " + "".join("triples_%d-%d-%d " % r[:3] for r in rows) + "step = %d" % step


def _check_blocks(tag, blocks, frames, rows, interval, nb=BINS):
    """blocks[k] holds the counts of frames[0 .. k]"""
    assert len(blocks) == len(frames)
    typ = H.types_from_species(frames[0]["species"], SYMBOLS)
    width = 180.0 / nb
    counts, amb = np.zeros((len(rows), nb), dtype=np.int64), np.zeros((len(rows), nb), dtype=np.int64)
    for k, (fr, (header, values)) in enumerate(zip(frames, blocks)):
        assert np.abs(fr["pos"]).max() < 100.0  # (nine digits: seven decimals from 10 A on)
        c, a = AK.expected_counts(np.ascontiguousarray(fr["pos"].T), typ, fr["h"], fr["pbc"], rows, nb, delta=DELTA)
        counts += c
        amb += a
        assert counts.sum() > 0 and amb.sum() <= 1e-3 * counts.sum(), (counts.sum(), amb.sum())
        assert header == _header(rows, (k + 1) * interval - 1), header
        assert values.shape == (nb, 1 + len(rows))
        assert np.allclose(values[:, 0], (np.arange(nb) + 0.5) * width, rtol=1e-5, atol=0.0)
        total, shaky = counts.sum(axis=1).astype(np.float64), amb.sum(axis=1).astype(np.float64)
        assert (total > 0).all()
        exp = counts / (total * width)[:, None]
        # an ambiguous triplet moves one count between two bins, or (a leg on a bound) in or out of the row: the total moves too
        allow = (amb + counts * (shaky / total)[:, None]) / ((total - shaky) * width)[:, None]
        dev = np.abs(values[:, 1:].T - exp)
        print("\n[%s block %d] largest deviation %.2e of %.3e, bins with an allowance %d" % (tag, k, dev.max(), exp.max(), int((amb > 0).sum())))
        assert (dev <= 1e-5 * exp + allow).all(), np.argwhere(dev > 1e-5 * exp + allow)[:5]


def _self_consistency(exe, tmp_path, replicate):
    for sub, line, rows in (("g", GLOBAL_LINE, GLOBAL_ROWS), ("t", TRIPLE_LINE, TRIPLE_ROWS)):
        wd = HR._workdir(tmp_path / sub, replicate + HEAD + line + "\ndump_xyz 5 d.xyz\nrun 10\n")
        out = HR._run(exe, wd)
        expected = ["Compute angular distribution functions (ADF).", "    ADF sample interval is 5 step.",
                    "    radial cutoff will be divided into 90 bins."]
        if rows is GLOBAL_ROWS:
            expected += ["    Global ADF will be computed.", "    minimal radial cutoff 0.", "    maximum radial cutoff 4."]
        else:
            expected += ["    Local triple ADF will be computed.", "    Triple 0-1-1: 2 5 2 5.", "    Triple 1-0-0: 2 5 2 5.",
                         "    Triple 0-0-1: 2 5 2 5."]
        for text in expected:
            assert text in out, (text, out[-2000:])
        frames = H.read_xyz_frames(os.path.join(wd, "d.xyz"))
        assert len(frames) == 2
        _check_blocks("%s %s" % (os.path.basename(exe), sub), HR._blocks(os.path.join(wd, "adf.out")), frames, rows, 5)


def test_adf_against_the_dumped_frames_on_emulator(tmp_path):
    _self_consistency(EMU, tmp_path, "replicate 2 2 2\n")


@pytest.mark.gpu
def test_adf_against_the_dumped_frames_on_gpu(tmp_path):
    _self_consistency(EXE, tmp_path, "replicate 3 3 3\n")


def test_two_runs_append_and_the_keyword_does_not_propagate_on_emulator(tmp_path):
    """a second `run` has a handle of its own and appends its blocks; the third has no compute_adf.  12 steps at interval 5: two blocks"""
    wd = HR._workdir(tmp_path, "replicate 2 2 2\n" + HEAD + GLOBAL_LINE + "\ndump_xyz 5 d.xyz\nrun 10\n"
                     + TRIPLE_LINE + "\ndump_xyz 5 d.xyz\nrun 12\nrun 3\n")
    HR._run(EMU, wd)
    frames = H.read_xyz_frames(os.path.join(wd, "d.xyz"))
    assert len(frames) == 4
    blocks = HR._blocks(os.path.join(wd, "adf.out"))
    assert len(blocks) == 4
    _check_blocks("first run", blocks[:2], frames[:2], GLOBAL_ROWS, 5)
    _check_blocks("second run", blocks[2:], frames[2:], TRIPLE_ROWS, 5)


T0 = "compute_adf 5 90 "


@pytest.mark.parametrize("line, message", [
    ("compute_adf 5 90 0", "compute_rdf should have at least 4 parameters."),
    ("compute_adf 5 90 0 1 1 2 5 2", "compute_adf should have 4 parameters or 2 + 7 * Ntriples parameters."),
    ("compute_adf x 90 0 4", "interval step per sample should be an integer."),
    ("compute_adf 0 90 0 4", "interval step per sample should be positive."),
    ("compute_adf 5 1.5 0 4", "number of bins should be an integer."),
    ("compute_adf 5 90 x 4", "minimum radial cutoff should be a number."),
    ("compute_adf 5 90 0 x", "maximum radial cutoff should be a number."),
    ("compute_adf 5 90 4 4", "minimum radial cutoff should be less than maximum radial cutoff."),
    ("compute_adf 5 90 -1 4", "minimum radial cutoff should be positive."),
    ("compute_adf 5 90 0 16", "The box has a thickness < 2.5 RDF radial cutoffs in a periodic direction."),
    ("compute_adf x 90 0 1 1 2 5 2 5", "interval step per sample should be an integer."),
    ("compute_adf 0 90 0 1 1 2 5 2 5", "interval step per sample should be positive."),
    ("compute_adf 5 1.5 0 1 1 2 5 2 5", "number of bins should be an integer."),
    (T0 + "x 1 1 2 5 2 5", "itype in triples 0 should be an integer."),
    (T0 + "-1 1 1 2 5 2 5", "itype in triples 0 should be non-negative."),
    (T0 + "2 1 1 2 5 2 5", "itype in triples 0 should be less than number of atomic types 2."),
    (T0 + "0 x 1 2 5 2 5", "jtype in triples 0 should be an integer."),
    (T0 + "0 -1 1 2 5 2 5", "jtype in triples 0 should be non-negative."),
    (T0 + "0 2 1 2 5 2 5", "jtype in triples 0 should be less than number of atomic types 2."),
    (T0 + "0 1 1 2 5 2 5 0 1 x 2 5 2 5", "ktype in triples 1 should be an integer."),
    (T0 + "0 1 1 2 5 2 5 0 1 -1 2 5 2 5", "ktype in triples 1 should be non-negative."),
    (T0 + "0 1 1 2 5 2 5 0 1 2 2 5 2 5", "ktype in triples 1 should be less than number of atomic types 2."),
    (T0 + "0 1 1 x 5 2 5", "minimum radial cutoff in triples 0 should be a number."),
    (T0 + "0 1 1 2 x 2 5", "maximum radial cutoff in triples 0 should be a number."),
    (T0 + "0 1 1 5 5 2 5", "minimum radial cutoff should be less than maximum radial cutoff for triples 0."),
    (T0 + "0 1 1 -1 5 2 5", "minimum radial cutoff in triples 0 should be positive."),
    (T0 + "0 1 1 2 5 x 5", "minimum radial cutoff in triples 0 should be a number."),
    (T0 + "0 1 1 2 5 2 x", "maximum radial cutoff in triples 0 should be a number."),
    (T0 + "0 1 1 2 5 6 5", "minimum radial cutoff should be less than maximum radial cutoff for triples 0."),
    (T0 + "0 1 1 2 5 -2 5", "minimum radial cutoff in triples 0 should be positive."),
    (T0 + "0 1 1 2 5 2 16", "The box has a thickness < 2.5 RDF radial cutoffs in a periodic direction."),
    # ours
    (T0 + "0 4\ncompute_adf 5 90 0 4", "compute_adf can be used once in a run."),
    (T0 + "0 1 1 2 5 2 5 " * 33, "compute_adf takes at most 32 triples."),
    ("compute_adf 5 0 0 4", "number of bins should be 1 to 4096."),
])
def test_input_errors_have_the_reference_messages(tmp_path, line, message):
    wd = HR._workdir(tmp_path, "replicate 2 2 2\n" + HEAD + line + "\nrun 10\n")
    HR._run(EMU, wd, expect_error=message, args=("--check-input",))


def test_thirty_two_triples_are_accepted(tmp_path):
    wd = HR._workdir(tmp_path, "replicate 2 2 2\n" + HEAD + T0 + "0 1 1 2 5 2 5 " * 32 + "\nrun 10\n")
    out = HR._run(EMU, wd, args=("--check-input",))
    assert out.count("    Triple 0-1-1: 2 5 2 5.") == 32


def test_an_overflowed_handle_ends_the_run_with_the_capacity(tmp_path):
    """rc = 14 A in PbTe (0.03 atoms / A^3): about 340 neighbours, above the capacity"""
    wd = HR._workdir(tmp_path, "replicate 2 2 2\n" + HEAD + "compute_adf 1 90 0 14\nrun 2\n")
    cap = (80 * 1024 // 2) // (4 * 32)
    HR._run(EMU, wd, expect_error="compute_adf: an atom has more than %d neighbours" % cap)
    assert not os.path.exists(os.path.join(wd, "adf.out")) or os.path.getsize(os.path.join(wd, "adf.out")) == 0


def test_multi_rank_launch_refuses(tmp_path):
    wd = HR._workdir(tmp_path, "replicate 4 2 2\npotential NEP x\nvelocity 300 seed 7\nensemble nve\ntime_step 1\ncompute_adf 2 90 0 4\nrun 4\n")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   NEPMI_TRANSPORT="tcp", OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([EMU], cwd=wd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode != 0 for p in procs), outs[0][-2000:]
    assert "compute_adf is not available in multi-GPU runs" in outs[0], outs[0][-2000:]
