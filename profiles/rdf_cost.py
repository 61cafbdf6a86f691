#!/usr/bin/env python3
"""What sampling g(r) inside the run loop costs: `compute_rdf 8 200 10`, NVE, 300 K, 1 fs, one engine per variant, alternating
rounds in one process, for
  PbTe   1,024,000 atoms (the 250-atom cell 16 x 16 x 16): two types, 3 x 200 bins = 2.4 KB of table, the LDS form;
  UNEP   256,000 atoms (fcc alloy 40 x 40 x 40, sixteen types): 136 x 200 bins = 109 KB, the form with global integer atomics.

  (a) nepmi_run_nve ms/step with nothing attached and with the RDF handle attached, three alternating rounds: median (min .. max);
      the difference x 10 is the cost of one sample (binning, scan, fill, pair kernel, accumulate);
  (b) one sample alone through nepmi_rdf_sample, timed with events on the engine's stream, with the number of pairs it counted
      and the number of candidate pairs the blocks' windows make it test;
  (c) where oracle/_ref/gpumd_ref exists: the reference's own program and gpumd-mi on the same input with and without the keyword,
      as cost per sample: (time with - time without) / samples.

Measured, not asserted.

    python profiles/rdf_cost.py [--reps 16] [--steps 200] [--rounds 3] [--out profiles/rdf_cost.json]
"""
import argparse
import json
import os
import shutil
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
RC, BINS, INTERVAL = 8.0, 200, 10


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), rounds=[float(x) for x in v])


def fmt(s):
    return "%.4f (%.4f .. %.4f)" % (s["median"], s["min"], s["max"])


def in_process(drv, torch, name, nep, h, typ, x, mass, num_types, args, out):
    import helpers as H
    from gpumd_amd.nep import RDF
    n = len(typ)
    vel = H.maxwell_velocities(mass, 300.0, seed=4)
    dt = 1.0 / H.TIME_UNIT
    model = drv.model(nep)
    res = out[name] = dict(atoms=n, num_types=num_types, rc=RC, num_bins=BINS, interval=INTERVAL, steps_per_round=args.steps)

    def fresh(with_rdf):
        eng = drv.engine(model, n)
        st = dict(t=drv.dev(typ), m=drv.dev(mass), x=drv.dev(x), v=drv.dev(vel), pe=drv.zeros(n), f=drv.zeros(3 * n), w=drv.zeros(9 * n))
        rdf = None
        if with_rdf:
            rdf = RDF(eng, RC, BINS, INTERVAL, typ, num_types)
            eng.attach(rdf)
        eng.force_compute(h, st["t"], st["x"], st["pe"], st["f"], st["w"])
        return eng, st, rdf

    def run(eng, st, steps):
        eng.run_nve(h, st["t"], st["m"], dt, steps, st["x"], st["v"], st["pe"], st["f"], st["w"], thermo_every=steps)

    variants = {"nothing_attached": fresh(False), "compute_rdf_8_200_10": fresh(True)}
    ms = {k: [] for k in variants}
    for eng, st, _ in variants.values():
        run(eng, st, args.warmup)
    for _ in range(args.rounds):
        for key, (eng, st, _) in variants.items():
            drv.sync()
            t0 = time.perf_counter()
            run(eng, st, args.steps)
            drv.sync()
            ms[key].append((time.perf_counter() - t0) * 1e3 / args.steps)
    res["run_nve_ms_per_step"] = {k: spread(v) for k, v in ms.items()}
    per = [(a - b) * INTERVAL for a, b in zip(ms["compute_rdf_8_200_10"], ms["nothing_attached"])]
    res["ms_per_sample_in_the_loop"] = spread(per)
    base = res["run_nve_ms_per_step"]["nothing_attached"]["median"]
    res["added_per_step_percent"] = 100.0 * (res["run_nve_ms_per_step"]["compute_rdf_8_200_10"]["median"] / base - 1.0)
    eng, st, rdf = variants["compute_rdf_8_200_10"]
    res["form"] = rdf.form
    res["samples_in_the_loop"] = rdf.read()[2]
    res["describe"] = eng.describe()
    print("[%s, %d atoms, form %d] run_nve ms/step: nothing attached %s, compute_rdf %g %d %d %s -> %+.1f %% per step, %s ms per sample"
          % (name, n, rdf.form, fmt(res["run_nve_ms_per_step"]["nothing_attached"]), RC, BINS, INTERVAL,
             fmt(res["run_nve_ms_per_step"]["compute_rdf_8_200_10"]), res["added_per_step_percent"], fmt(res["ms_per_sample_in_the_loop"])))

    # (b) one sample alone
    eng0, st0, _ = variants["nothing_attached"]
    one = RDF(eng0, RC, BINS, 1, typ, num_types)
    one.sample(st0["x"], h, (1, 1, 1))
    counts, _, _ = one.read()
    t = []
    for _ in range(3 * args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        one.sample(st0["x"], h, (1, 1, 1))
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    one.close()
    s = spread(t)
    pairs = int(counts.sum())
    # candidates: every centre atom against the atoms of its block's window, (4 + 4)^3 cells of edge >= rc / 2
    Hm = np.asarray(h).reshape(3, 3)
    vol = abs(np.linalg.det(Hm))
    thick = [vol / np.linalg.norm(np.cross(Hm[:, (d + 1) % 3], Hm[:, (d + 2) % 3])) for d in range(3)]
    cells = [int(np.floor(tk / (0.5 * RC))) for tk in thick]
    per_cell = n / float(np.prod(cells))
    candidates = n * per_cell * 512.0
    s.update(pairs_counted=pairs, candidate_pairs=candidates, candidates_per_ns=candidates / (s["median"] * 1e6),
             hits_per_ns=pairs / (s["median"] * 1e6), cells=cells)
    res["one_sample"] = s
    print("[%s] one sample through nepmi_rdf_sample: %s ms; %.3g pairs counted of %.3g candidates (%.1f x): %.1f candidates / ns, "
          "%.2f hits / ns" % (name, fmt(s), pairs, candidates, candidates / max(pairs, 1), s["candidates_per_ns"], s["hits_per_ns"]))
    for eng, st, rdf in variants.values():
        if rdf is not None:
            rdf.close()
        eng.close()
    del variants
    torch.cuda.empty_cache()


def binaries(name, case_writer, args, out, steps):
    import ref_compare as R
    if not os.path.exists(R.REF):
        print("oracle/_ref/gpumd_ref is not built: the reference's cost per sample is not measured")
        out.setdefault("not_measured", []).append(name + ": reference binary (not built)")
        return
    samples = steps // INTERVAL
    configs = {"none": "", "rdf": "compute_rdf %g %d %d\n" % (RC, BINS, INTERVAL)}
    res = {exe: {k: [] for k in configs} for exe in ("gpumd_ref", "gpumd_mi")}
    base = os.path.join(args.scratch, "rdf_cost_runs")
    for rnd in range(args.rounds):
        for key, extra in configs.items():
            for tag, exe in (("gpumd_ref", R.REF), ("gpumd_mi", R.MI)):
                d = os.path.join(base, "%s_%s" % (tag, key))
                shutil.rmtree(d, ignore_errors=True)
                os.makedirs(d)
                case_writer(R, d, extra, steps)
                r, _ = R.run_binary(exe, d, 900.0)
                if r["rc"] != 0 or r["run_seconds"] is None:
                    raise SystemExit("%s failed on %s: see %s/stdout.txt" % (tag, key, d))
                res[tag][key].append(r["run_seconds"])
                print("  round %d %-9s %-4s %.3f s" % (rnd, tag, key, r["run_seconds"]), flush=True)
    shutil.rmtree(base, ignore_errors=True)
    o = out[name]["binaries"] = dict(steps=steps, samples=samples)
    for tag in res:
        q = {k: spread(v) for k, v in res[tag].items()}
        q["ms_per_sample"] = spread([(a - b) * 1e3 / samples for a, b in zip(res[tag]["rdf"], res[tag]["none"])])
        o[tag] = q
        print("[%s] %-9s run of %d steps: none %.3f s, compute_rdf %.3f s -> %s ms per sample"
              % (name, tag, steps, q["none"]["median"], q["rdf"]["median"], fmt(q["ms_per_sample"])))


def pbte_case(reps):
    def write(R, d, extra, steps):
        shutil.copy(os.path.join(R.GOLD, "PbTe", "model.xyz"), os.path.join(d, "model.xyz"))
        shutil.copy(os.path.join(R.GOLD, "PbTe", "nep.txt"), os.path.join(d, "nep.txt"))
        with open(os.path.join(d, "run.in"), "w") as f:
            f.write("replicate %d %d %d\npotential nep.txt\nvelocity 300\nensemble nve\ntime_step 1\n%srun %d\n" % (reps, reps, reps, extra, steps))
    return write


def unep_case(cells):
    def write(R, d, extra, steps):
        symbols = open(os.path.join(R.GOLD, "UNEP", "nep.txt")).readline().split()[2:]
        lat, spec, pos = R.fcc_alloy_cell(3.9, symbols, cells)
        R.write_xyz(os.path.join(d, "model.xyz"), lat, spec, pos)
        shutil.copy(os.path.join(R.GOLD, "UNEP", "nep.txt"), os.path.join(d, "nep.txt"))
        with open(os.path.join(d, "run.in"), "w") as f:
            f.write("potential nep.txt\nvelocity 300\nensemble nve\ntime_step 1\n%srun %d\n" % (extra, steps))
    return write


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--unep-cells", type=int, default=40)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ref-steps", type=int, default=300)
    ap.add_argument("--unep-ref-steps", type=int, default=100)
    ap.add_argument("--no-binaries", action="store_true")
    ap.add_argument("--no-unep", action="store_true")
    ap.add_argument("--scratch", default=os.path.join(ROOT, "bench_out"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rdf_cost.json"))
    args = ap.parse_args()
    import torch
    import helpers as H
    drv = H.GpuDriver()
    out = dict(rounds=args.rounds)

    h, typ, x = H.pbte_supercell((args.reps,) * 3, rattle=0.03, seed=17)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    in_process(drv, torch, "pbte", H.golden("PbTe", "nep.txt"), h, typ, x, mass, 2, args, out)
    if not args.no_binaries:
        binaries("pbte", pbte_case(args.reps), args, out, args.ref_steps)
    if not args.no_unep:
        h, typ, x = H.fcc_alloy((args.unep_cells,) * 3, 3.9, 16, rattle=0.02, seed=5)
        in_process(drv, torch, "unep", H.golden("UNEP", "nep.txt"), h, typ, x, np.full(len(typ), 100.0), 16, args, out)
        if not args.no_binaries:
            binaries("unep", unep_case(args.unep_cells), args, out, args.unep_ref_steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("written: " + args.out)


if __name__ == "__main__":
    main()
