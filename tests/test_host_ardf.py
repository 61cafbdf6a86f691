"""`compute_angular_rdf <rc> <r_bins> <theta_bins> <interval> [atom i j]...` in gpumd-mi (gpumd_amd/host/run.cpp): the run dumps
its frames with `dump_xyz` at the sample interval and angular_rdf.out is recomputed from them in numpy -- all ordered pairs,
minimum image, the bin rule of include/nepmi.h (test_run_ardf.expected_counts), then the one normalisation: per sample
V / (N^2 bv) per ordered pair for the total, V / (N_a^2 bv) for (a, a), V / (N_a N_b bv) per a -> b pair for (a, b),
bv = D / (2 pi) * 4 pi / 3 (up^3 - lo^3), divided by number_of_steps / interval.

Tolerance.  dump_xyz prints nine significant digits: coordinates of 10 .. 100 A are rounded by at most delta = 5e-8 A.  A pair
within delta of an r edge, or within delta / (its in-plane distance) of a theta edge, is ambiguous; asserted first: they are at
most 1e-3 of the counted pairs.  Every printed number within 1e-5 (the `%.5f` quantum) plus the ambiguous pairs' weight in that
bin and column.  The header line as text.

CPU tier: the host linked against the kernel emulator (tests/emu/gpumd-mi-emu), the 250-atom PbTe cell replicated 2 x 2 x 2
(resident loop) and unreplicated (19 A thick: the small-box loop, which steps on the host's arrays); one GPU case with the product
binary on 3 x 3 x 3.  Input errors through --check-input."""
import os
import shutil
import socket
import subprocess

import numpy as np
import pytest

import helpers as H
import test_rdf_kernels as RK
import test_run_ardf as RA

EMU = os.path.join(H.ROOT, "tests", "emu", "gpumd-mi-emu")
EXE = os.path.join(H.ROOT, "gpumd_amd", "bin", "gpumd-mi")
HEAD = "potential NEP\nvelocity 1500 seed 7\nensemble nve\ntime_step 2\n"
DELTA = 5e-8
SYMBOLS = ["Te", "Pb"]  # the potential's order
P3 = ((0, 0), (0, 1), (1, 1))
GROUPS = " atom 0 0 atom 0 1 atom 1 1"


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(H.ROOT, "tests", "emu"), "all"], check=True)


def _workdir(tmp_path, run_in):
    os.makedirs(str(tmp_path), exist_ok=True)
    shutil.copy(H.golden("PbTe", "model.xyz"), os.path.join(str(tmp_path), "model.xyz"))
    with open(os.path.join(str(tmp_path), "run.in"), "w") as f:
        f.write(run_in.replace("NEP", H.golden("PbTe", "nep.txt")))
    return str(tmp_path)


def _run(exe, wd, expect_error=None, args=()):
    res = subprocess.run([exe, *args], cwd=wd, capture_output=True, text=True, timeout=600)
    if expect_error is None:
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    else:
        assert res.returncode != 0 and expect_error in res.stdout + res.stderr, (expect_error, res.stdout[-1500:] + res.stderr[-500:])
    return res.stdout


def _blocks(path):
    out = []
    for line in open(path).read().splitlines():
        if line.startswith("#"):
            out.append((line, []))
        else:
            out[-1][1].append([float(x) for x in line.split()])
    return [(h, np.array(r)) for h, r in out]


def _expected_rows(frames, rc, R, T, pairs, num_repeats):
    """-> rows [R * T, 2 + C] like angular_rdf.out (r outer, theta inner), allowance (the ambiguous pairs' weight)"""
    from gpumd_amd.nep import ardf_normalise
    typ = H.types_from_species(frames[0]["species"], SYMBOLS)
    na = np.array([(typ == 0).sum(), (typ == 1).sum()], dtype=np.float64)
    C = 1 + len(pairs)
    cv, av = np.zeros((C, R, T)), np.zeros((C, R, T))
    counted = ambiguous = 0
    for fr in frames:
        assert np.abs(fr["pos"]).max() < 100.0  # (nine digits: seven decimals from 10 A on)
        c, a = RA.expected_counts(np.ascontiguousarray(fr["pos"].T), typ, fr["h"], fr["pbc"], rc, R, T, pairs, DELTA)
        V = RK.box_volume(fr["h"])
        counted += c[0].sum()
        ambiguous += a[0].sum()
        cv += c * V
        av += a * V
    assert counted > 0 and ambiguous <= 1e-3 * counted, (counted, ambiguous)
    r, th, g = ardf_normalise(cv, rc, pairs, na, num_repeats)
    _, _, ga = ardf_normalise(av, rc, pairs, na, num_repeats)
    rows, allow = np.zeros((R * T, 2 + C)), np.zeros((R * T, 2 + C))
    rows[:, 0], rows[:, 1] = np.repeat(r, T), np.tile(th, R)
    rows[:, 2:] = g.reshape(C, R * T).T
    allow[:, 2:] = ga.reshape(C, R * T).T
    return rows, allow


def _check_block(tag, block, frames, rc, R, T, pairs, num_repeats):
    header, values = block
    assert header == "#radius theta total" + "".join(" type_%d_%d" % p for p in pairs), header
    exp, allow = _expected_rows(frames, rc, R, T, pairs, num_repeats)
    assert values.shape == exp.shape
    dev = np.abs(values - exp)
    print("\n[%s] angular_rdf.out: largest deviation %.2e (quantum 1e-5), largest g %.3f, entries with an allowance %d"
          % (tag, dev.max(), exp[:, 2:].max(), int((allow > 0).sum())))
    assert exp[:, 2].max() > 1.0  # a crystal's first shells stand out: the numbers are not trivially zero
    assert (dev <= 1.0e-5 + allow).all(), np.argwhere(dev > 1.0e-5 + allow)[:5]


def _self_consistency(exe, tmp_path, replicate, rc, R, groups, pairs):
    wd = _workdir(tmp_path, replicate + HEAD + "compute_angular_rdf %g %d 24 5%s\ndump_xyz 5 d.xyz\nrun 10\n" % (rc, R, groups))
    out = _run(exe, wd)
    for line in ("Compute Angular RDF.", "    radial cutoff %g." % rc, "    radial cutoff will be divided into %d bins." % R,
                 "    theta cutoff will be divided into 24 bins.", "    Angular RDF sample interval is 5 step."):
        assert line in out, (line, out[-2000:])
    frames = H.read_xyz_frames(os.path.join(wd, "d.xyz"))
    assert len(frames) == 2
    (block,) = _blocks(os.path.join(wd, "angular_rdf.out"))
    _check_block("%s n=%d" % (os.path.basename(exe), frames[0]["n"]), block, frames, rc, R, 24, pairs, 2)


def test_total_only_against_the_dumped_frames_on_emulator(tmp_path):
    _self_consistency(EMU, tmp_path, "replicate 2 2 2\n", 8.0, 40, "", ())


def test_three_atom_groups_against_the_dumped_frames_on_emulator(tmp_path):
    _self_consistency(EMU, tmp_path, "replicate 2 2 2\n", 8.0, 40, GROUPS, P3)


def test_small_box_stepwise_path_on_emulator(tmp_path):
    """the unreplicated cell: 19 A thick, below 2.5 (rc + skin) of the potential, so the host's arrays are stepped call by call"""
    _self_consistency(EMU, tmp_path, "", 7.0, 35, GROUPS, P3)


@pytest.mark.gpu
def test_three_atom_groups_against_the_dumped_frames_on_gpu(tmp_path):
    _self_consistency(EXE, tmp_path, "replicate 3 3 3\n", 8.0, 40, GROUPS, P3)


def test_two_runs_append_and_the_keyword_does_not_propagate_on_emulator(tmp_path):
    """a second `run` appends its own block; the third has no compute_angular_rdf.  12 steps at interval 5: two samples, and
    num_repeats = 12 / 5 = 2"""
    wd = _workdir(tmp_path, "replicate 2 2 2\n" + HEAD + "compute_angular_rdf 8 40 24 5\ndump_xyz 5 d.xyz\nrun 10\n"
                  "compute_angular_rdf 6 30 21 5 atom 0 1\ndump_xyz 5 d.xyz\nrun 12\nrun 3\n")
    _run(EMU, wd)
    frames = H.read_xyz_frames(os.path.join(wd, "d.xyz"))
    assert len(frames) == 4
    blocks = _blocks(os.path.join(wd, "angular_rdf.out"))
    assert len(blocks) == 2 and len(blocks[0][1]) == 40 * 24 and len(blocks[1][1]) == 30 * 21
    _check_block("first run", blocks[0], frames[:2], 8.0, 40, 24, (), 2)
    _check_block("second run", blocks[1], frames[2:], 6.0, 30, 21, ((0, 1),), 2)


@pytest.mark.parametrize("line, message", [
    ("compute_angular_rdf 8 40 24", "compute_angular_rdf should have at least 4 parameters."),
    ("compute_angular_rdf 8 40 24 5" + " atom 0 0" * 6 + " atom", "compute_angular_rdf has too many parameters."),
    ("compute_angular_rdf x 40 24 5", "radial cutoff should be a number."),
    ("compute_angular_rdf 0 40 24 5", "radial cutoff should be positive."),
    ("compute_angular_rdf 16 40 24 5", "The box has a thickness < 2.5 RDF radial cutoffs in a periodic direction."),
    ("compute_angular_rdf 8 1.5 24 5", "number of bins should be an integer."),
    ("compute_angular_rdf 8 20 24 5", "A larger nbins is recommended."),
    ("compute_angular_rdf 8 501 24 5", "A smaller nbins is recommended."),
    ("compute_angular_rdf 8 40 x 5", "number of theta bins should be an integer."),
    ("compute_angular_rdf 8 40 20 5", "A larger ntheta is recommended."),
    ("compute_angular_rdf 8 40 24 x", "interval step per sample should be an integer."),
    ("compute_angular_rdf 8 40 24 0", "interval step per sample should be positive."),
    ("compute_angular_rdf 8 40 24 5 atoms 0 1", "Unrecognized argument in compute_angular_rdf."),
    ("compute_angular_rdf 8 40 24 5 atom x 1", "atom type index1 should be an integer."),
    ("compute_angular_rdf 8 40 24 5 atom -1 1", "atom type index1 should be non-negative."),
    ("compute_angular_rdf 8 40 24 5 atom 3 1", "atom type index1 should be less than number of atomic types."),
    ("compute_angular_rdf 8 40 24 5 atom 0 x", "atom type index2 should be an integer."),
    ("compute_angular_rdf 8 40 24 5 atom 0 -1", "atom type index2 should be non-negative."),
    ("compute_angular_rdf 8 40 24 5 atom 0 3", "atom type index1 should be less than number of atomic types."),  # (sic)
    # ours: a type index EQUAL to the number of types (the reference's test is >), a trailing group without its numbers, and the
    # library's limit of theta bins
    ("compute_angular_rdf 8 40 24 5 atom 2 1", "atom type index1 should be less than number of atomic types."),
    ("compute_angular_rdf 8 40 24 5 atom 0 2", "atom type index1 should be less than number of atomic types."),
    ("compute_angular_rdf 8 40 24 5 atom 0 0 atom 1", "an atom group of compute_angular_rdf should have 2 type indices."),
    ("compute_angular_rdf 8 40 24 5 atom", "an atom group of compute_angular_rdf should have 2 type indices."),
    ("compute_angular_rdf 8 40 1025 5", "number of theta bins should be at most 1024."),
])
def test_input_errors_have_the_reference_messages(tmp_path, line, message):
    wd = _workdir(tmp_path, "replicate 2 2 2\n" + HEAD + line + "\nrun 10\n")
    _run(EMU, wd, expect_error=message, args=("--check-input",))


def test_the_unreplicated_cell_is_too_thin(tmp_path):
    """19 A thick: rc = 8 A asks for 20 A"""
    wd = _workdir(tmp_path, HEAD + "compute_angular_rdf 8 40 24 5\nrun 10\n")
    _run(EMU, wd, expect_error="Please increase the periodic direction(s).", args=("--check-input",))
    ok = _workdir(tmp_path / "ok", HEAD + "compute_angular_rdf 7 40 24 5\nrun 10\n")
    out = _run(EMU, ok, args=("--check-input",))
    assert "    radial cutoff 7." in out


def test_multi_rank_launch_refuses(tmp_path):
    wd = _workdir(tmp_path, "replicate 4 2 2\npotential NEP x\nvelocity 300 seed 7\nensemble nve\ntime_step 1\n"
                  "compute_angular_rdf 8 40 24 2\nrun 4\n")
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
    assert "compute_angular_rdf is not available in multi-GPU runs" in outs[0], outs[0][-2000:]
