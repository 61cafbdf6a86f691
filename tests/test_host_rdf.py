"""`compute_rdf <rc> <num_bins> <interval>` in gpumd-mi (gpumd_amd/host/run.cpp): the run dumps its frames with `dump_xyz` at the
sample interval and rdf.out is recomputed from them in numpy -- all pairs, minimum image, the bin rule of rdf.cu:97-118
(test_rdf_kernels.expected_counts), then RDF::postprocess: per sample 2 V / (N^2 dV) per unordered pair for the total,
2 V / (N_a^2 dV) and V / (N_a N_b dV) for the partials, dV = 4 pi ((w + 0.5) dr)^2 dr, divided by number_of_steps / interval.

Tolerance.  dump_xyz prints nine significant digits: coordinates of 10 .. 100 A are rounded by at most delta = 5e-8 A, half a unit
of the last digit.  A pair whose distance lies within delta of a bin edge or of rc is ambiguous; asserted first: they are at most
1e-3 of the counted pairs.  Every printed number within 1e-5 (the `%.5f` quantum) plus the ambiguous pairs' weight in that bin
and column.  The header line as text.

CPU tier: the host linked against the kernel emulator (tests/emu/gpumd-mi-emu), the 250-atom PbTe cell replicated 2 x 2 x 2 (38 A
thick: 2.5 x 8 A fits); one GPU case with the product binary on 3 x 3 x 3.  Input errors through --check-input."""
import os
import shutil
import socket
import subprocess

import numpy as np
import pytest

import helpers as H
import test_rdf_kernels as RK

EMU = os.path.join(H.ROOT, "tests", "emu", "gpumd-mi-emu")
EXE = os.path.join(H.ROOT, "gpumd_amd", "bin", "gpumd-mi")
HEAD = "potential NEP\nvelocity 1500 seed 7\nensemble nve\ntime_step 2\n"
DELTA = 5e-8
SYMBOLS = ["Te", "Pb"]  # the potential's order


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


def _expected_rows(frames, rc, nb, num_repeats):
    """-> rows [nb, 5] like rdf.out, allowance [nb, 5] (the ambiguous pairs' weight; 0 for the radius)"""
    typ = H.types_from_species(frames[0]["species"], SYMBOLS)
    n = len(typ)
    na = np.array([(typ == 0).sum(), (typ == 1).sum()], dtype=np.float64)
    dr = rc / nb
    r = (np.arange(nb) + 0.5) * dr
    dV = 4.0 * np.pi * r * r * dr
    rows, allow = np.zeros((nb, 5)), np.zeros((nb, 5))
    rows[:, 0] = r
    counted = ambiguous = 0
    for fr in frames:
        assert np.abs(fr["pos"]).max() < 100.0  # (nine digits: seven decimals from 10 A on)
        c, a = RK.expected_counts(np.ascontiguousarray(fr["pos"].T), typ, fr["h"], fr["pbc"], rc, nb, 2, eps_abs=DELTA)
        V = RK.box_volume(fr["h"])
        counted += c.sum()
        ambiguous += a.sum()
        for tab, out in ((c, rows), (a, allow)):
            out[:, 1] += 2.0 * V * tab.sum(axis=0) / (n * n * dV)
            out[:, 2] += 2.0 * V * tab[0] / (na[0] * na[0] * dV)
            out[:, 3] += V * tab[1] / (na[0] * na[1] * dV)
            out[:, 4] += 2.0 * V * tab[2] / (na[1] * na[1] * dV)
    assert counted > 0 and ambiguous <= 1e-3 * counted, (counted, ambiguous)
    rows[:, 1:] /= num_repeats
    allow[:, 1:] /= num_repeats
    return rows, allow


def _check_block(tag, block, frames, rc, nb, num_repeats):
    header, values = block
    assert header == "#radius total Te-Te Te-Pb Pb-Pb", header
    exp, allow = _expected_rows(frames, rc, nb, num_repeats)
    assert values.shape == exp.shape
    dev = np.abs(values - exp)
    print("\n[%s] rdf.out: largest deviation %.2e (quantum 1e-5), largest g %.3f, bins with an allowance %d"
          % (tag, dev.max(), exp[:, 1:].max(), int((allow > 0).sum())))
    assert exp[:, 1].max() > 1.0  # a crystal's first shells stand out: the numbers are not trivially zero
    assert (dev <= 1.0e-5 + allow).all(), np.argwhere(dev > 1.0e-5 + allow)[:5]


def _self_consistency(exe, tmp_path, replicate):
    wd = _workdir(tmp_path, replicate + HEAD + "compute_rdf 8 100 5\ndump_xyz 5 d.xyz\nrun 10\n")
    out = _run(exe, wd)
    for line in ("Compute radial distribution function (RDF).", "    radial cutoff 8.", "    radial cutoff will be divided into 100 bins.",
                 "    RDF sample interval is 5 step.", "    There are 2 atom types in model.xyz.",
                 "    Will calculate one total RDF and 3 partial RDFs."):
        assert line in out, (line, out[-2000:])
    frames = H.read_xyz_frames(os.path.join(wd, "d.xyz"))
    n = frames[0]["n"]
    assert len(frames) == 2
    assert "        Type 0 has %d atoms." % (n // 2) in out and "        Type 1 has %d atoms." % (n // 2) in out
    (block,) = _blocks(os.path.join(wd, "rdf.out"))
    _check_block("%s n=%d" % (os.path.basename(exe), n), block, frames, 8.0, 100, 2)


def test_rdf_against_the_dumped_frames_on_emulator(tmp_path):
    _self_consistency(EMU, tmp_path, "replicate 2 2 2\n")


@pytest.mark.gpu
def test_rdf_against_the_dumped_frames_on_gpu(tmp_path):
    _self_consistency(EXE, tmp_path, "replicate 3 3 3\n")


def test_two_runs_append_and_the_keyword_does_not_propagate_on_emulator(tmp_path):
    """a second `run` appends its own block; the third has no compute_rdf.  12 steps at interval 5: two samples, and
    num_repeats = 12 / 5 = 2 in integer division (rdf.cu:236)"""
    wd = _workdir(tmp_path, "replicate 2 2 2\n" + HEAD + "compute_rdf 8 100 5\ndump_xyz 5 d.xyz\nrun 10\n"
                  "compute_rdf 6 40 5\ndump_xyz 5 d.xyz\nrun 12\nrun 3\n")
    _run(EMU, wd)
    frames = H.read_xyz_frames(os.path.join(wd, "d.xyz"))
    assert len(frames) == 4
    blocks = _blocks(os.path.join(wd, "rdf.out"))
    assert len(blocks) == 2 and len(blocks[0][1]) == 100 and len(blocks[1][1]) == 40
    _check_block("first run", blocks[0], frames[:2], 8.0, 100, 2)
    _check_block("second run", blocks[1], frames[2:], 6.0, 40, 2)


@pytest.mark.parametrize("line, message", [
    ("compute_rdf 8 100", "compute_rdf should have 3 parameters."),
    ("compute_rdf 8 100 5 1", "compute_rdf should have 3 parameters."),
    ("compute_rdf x 100 5", "radial cutoff should be a number."),
    ("compute_rdf 0 100 5", "radial cutoff should be positive."),
    ("compute_rdf -1 100 5", "radial cutoff should be positive."),
    ("compute_rdf 16 100 5", "The box has a thickness < 2.5 RDF radial cutoffs in a periodic direction."),
    ("compute_rdf 8 1.5 5", "number of bins should be an integer."),
    ("compute_rdf 8 20 5", "A larger nbins is recommended."),
    ("compute_rdf 8 501 5", "A smaller nbins is recommended."),
    ("compute_rdf 8 100 x", "interval step per sample should be an integer."),
    ("compute_rdf 8 100 0", "interval step per sample should be positive."),
])
def test_input_errors_have_the_reference_messages(tmp_path, line, message):
    wd = _workdir(tmp_path, "replicate 2 2 2\n" + HEAD + line + "\nrun 10\n")
    _run(EMU, wd, expect_error=message, args=("--check-input",))


def test_the_unreplicated_cell_is_too_thin(tmp_path):
    """19 A thick: rc = 8 A asks for 20 A"""
    wd = _workdir(tmp_path, HEAD + "compute_rdf 8 100 5\nrun 10\n")
    _run(EMU, wd, expect_error="Please increase the periodic direction(s).", args=("--check-input",))
    ok = _workdir(tmp_path / "ok", HEAD + "compute_rdf 7 100 5\nrun 10\n")
    out = _run(EMU, ok, args=("--check-input",))
    assert "    radial cutoff 7." in out


def test_multi_rank_launch_refuses(tmp_path):
    wd = _workdir(tmp_path, "replicate 4 2 2\npotential NEP x\nvelocity 300 seed 7\nensemble nve\ntime_step 1\ncompute_rdf 8 100 2\nrun 4\n")
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
    assert "compute_rdf is not available in multi-GPU runs" in outs[0], outs[0][-2000:]
