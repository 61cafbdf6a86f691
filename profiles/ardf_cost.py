#!/usr/bin/env python3
"""What sampling the angular-resolved RDF inside the run loop costs, beside compute_rdf on the same input in the same session:
PbTe 1,024,000 atoms (the 250-atom cell 16 x 16 x 16), NVE, 300 K, 1 fs, one engine per variant, alternating rounds in one
process, for
  compute_rdf 8 200 10                                        the yardstick: the same candidates, one bin dimension less
  compute_angular_rdf 8 200 36 10                             total only: 28.8 KB of table, the LDS form
  compute_angular_rdf 8 200 36 10 atom 0 0 atom 0 1 atom 1 1  four columns: 115 KB of table, the form the byte rule chooses

  (a) nepmi_run_nve ms/step with nothing attached and with each handle attached, alternating rounds: median (min .. max); the
      difference x 10 is the cost of one sample (binning, scan, fill, pair kernel, accumulate);
  (b) one sample alone through nepmi_rdf_sample / nepmi_ardf_sample, timed with events on the engine's stream, with the pairs
      counted;
  (c) with --ref and where oracle/_ref/gpumd_ref exists: the reference's own program and gpumd-mi with and without
      `compute_angular_rdf 8 40 24 10` at --ref-reps (default 10: 250,000 atoms; the reference keeps one double per atom and bin on
      the device and on the host), as cost per sample, with the reference's device memory from its own log where it prints it.

Measured, not asserted.

    python profiles/ardf_cost.py [--reps 16] [--steps 200] [--rounds 3] [--ref] [--out profiles/ardf_cost.json]
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
RC, RBINS, TBINS, INTERVAL = 8.0, 200, 36, 10
P3 = ((0, 0), (0, 1), (1, 1))


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), rounds=[float(x) for x in v])


def fmt(s):
    return "%.4f (%.4f .. %.4f)" % (s["median"], s["min"], s["max"])


def make(kind, eng, typ, interval):
    from gpumd_amd.nep import ARDF, RDF
    if kind == "compute_rdf":
        return RDF(eng, RC, RBINS, interval, typ, 2)
    return ARDF(eng, RC, RBINS, TBINS, interval, typ, 2, P3 if kind == "compute_angular_rdf_3_groups" else ())


KINDS = ("compute_rdf", "compute_angular_rdf", "compute_angular_rdf_3_groups")


def in_process(drv, torch, nep, h, typ, x, mass, args, out):
    import helpers as H
    n = len(typ)
    vel = H.maxwell_velocities(mass, 300.0, seed=4)
    dt = 1.0 / H.TIME_UNIT
    model = drv.model(nep)
    res = out["pbte"] = dict(atoms=n, rc=RC, r_bins=RBINS, theta_bins=TBINS, interval=INTERVAL, steps_per_round=args.steps)

    def fresh(kind):
        eng = drv.engine(model, n)
        st = dict(t=drv.dev(typ), m=drv.dev(mass), x=drv.dev(x), v=drv.dev(vel), pe=drv.zeros(n), f=drv.zeros(3 * n), w=drv.zeros(9 * n))
        handle = None
        if kind:
            handle = make(kind, eng, typ, INTERVAL)
            eng.attach(handle)
        eng.force_compute(h, st["t"], st["x"], st["pe"], st["f"], st["w"])
        return eng, st, handle

    def run(eng, st, steps):
        eng.run_nve(h, st["t"], st["m"], dt, steps, st["x"], st["v"], st["pe"], st["f"], st["w"], thermo_every=steps)

    variants = {"nothing_attached": fresh(None)}
    variants.update({k: fresh(k) for k in KINDS})
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
    base = res["run_nve_ms_per_step"]["nothing_attached"]
    print("[pbte, %d atoms] run_nve ms/step, nothing attached: %s" % (n, fmt(base)))
    res["in_the_loop"] = {}
    for k in KINDS:
        per = spread([(a - b) * INTERVAL for a, b in zip(ms[k], ms["nothing_attached"])])
        form = variants[k][2].form
        pct = 100.0 * (res["run_nve_ms_per_step"][k]["median"] / base["median"] - 1.0)
        res["in_the_loop"][k] = dict(ms_per_sample=per, form=form, added_per_step_percent=pct, samples=variants[k][2].read()[-1])
        print("[pbte] %-30s form %d: %s ms/step -> %+.1f %% per step, %s ms per sample"
              % (k, form, fmt(res["run_nve_ms_per_step"][k]), pct, fmt(per)))

    # (b) one sample alone
    eng0, st0, _ = variants["nothing_attached"]
    res["one_sample"] = {}
    for k in KINDS:
        one = make(k, eng0, typ, 1)
        one.sample(st0["x"], h, (1, 1, 1))
        counts = one.read()[0]
        t = []
        for _ in range(3 * args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            one.sample(st0["x"], h, (1, 1, 1))
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        form = one.form
        one.close()
        s = spread(t)
        s.update(form=form, counts_added=int(counts.sum()), unordered_pairs=int(counts[0].sum() // 2 if k != "compute_rdf" else counts.sum()))
        res["one_sample"][k] = s
        print("[pbte] one sample alone, %-30s form %d: %s ms; %.4g unordered pairs, %.4g table adds"
              % (k, form, fmt(s), s["unordered_pairs"], s["counts_added"] if k != "compute_rdf" else s["unordered_pairs"]))
    y = res["one_sample"]["compute_rdf"]["median"]
    for k in KINDS[1:]:
        res["one_sample"][k]["ratio_to_compute_rdf"] = res["one_sample"][k]["median"] / y
        print("[pbte] %s / compute_rdf, one sample alone: %.2f x" % (k, res["one_sample"][k]["ratio_to_compute_rdf"]))
    for eng, st, handle in variants.values():
        if handle is not None:
            handle.close()
        eng.close()
    del variants
    torch.cuda.empty_cache()


def binaries(args, out):
    import ref_compare as R
    if not os.path.exists(R.REF):
        print("oracle/_ref/gpumd_ref is not built: the reference's cost per sample is not measured")
        out.setdefault("not_measured", []).append("reference binary (not built)")
        return
    steps, reps = args.ref_steps, args.ref_reps
    samples = steps // INTERVAL
    keyword = "compute_angular_rdf %g 40 24 %d\n" % (RC, INTERVAL)
    configs = {"none": "", "ardf": keyword}
    res = {exe: {k: [] for k in configs} for exe in ("gpumd_ref", "gpumd_mi")}
    base = os.path.join(args.scratch, "ardf_cost_runs")
    for key, extra in configs.items():
        for tag, exe in (("gpumd_ref", R.REF), ("gpumd_mi", R.MI)):
            d = os.path.join(base, "%s_%s" % (tag, key))
            shutil.rmtree(d, ignore_errors=True)
            os.makedirs(d)
            shutil.copy(os.path.join(R.GOLD, "PbTe", "model.xyz"), os.path.join(d, "model.xyz"))
            shutil.copy(os.path.join(R.GOLD, "PbTe", "nep.txt"), os.path.join(d, "nep.txt"))
            with open(os.path.join(d, "run.in"), "w") as f:
                f.write("replicate %d %d %d\npotential nep.txt\nvelocity 300\nensemble nve\ntime_step 1\n%srun %d\n" % (reps, reps, reps, extra, steps))
            r, _ = R.run_binary(exe, d, 900.0)
            if r["rc"] != 0 or r["run_seconds"] is None:
                print("  %s failed on '%s' (rc %s): could not be run" % (tag, key, r["rc"]))
                out.setdefault("not_measured", []).append("%s %s: rc %s" % (tag, key, r["rc"]))
                continue
            res[tag][key].append(r["run_seconds"])
            print("  %-9s %-4s %.3f s" % (tag, key, r["run_seconds"]), flush=True)
    shutil.rmtree(base, ignore_errors=True)
    o = out["binaries"] = dict(steps=steps, samples=samples, atoms=250 * reps ** 3, keyword=keyword.strip(),
                               reference_table_bytes_per_column=250 * reps ** 3 * 40 * 24 * 8)
    for tag in res:
        if res[tag]["none"] and res[tag]["ardf"]:
            o[tag] = dict(none_s=res[tag]["none"][0], ardf_s=res[tag]["ardf"][0],
                          ms_per_sample=(res[tag]["ardf"][0] - res[tag]["none"][0]) * 1e3 / samples)
            print("[binaries, %d atoms] %-9s run of %d steps: none %.3f s, with the keyword %.3f s -> %.2f ms per sample"
                  % (o["atoms"], tag, steps, o[tag]["none_s"], o[tag]["ardf_s"], o[tag]["ms_per_sample"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ref", action="store_true")
    ap.add_argument("--ref-reps", type=int, default=10)
    ap.add_argument("--ref-steps", type=int, default=20)
    ap.add_argument("--scratch", default=os.path.join(ROOT, "bench_out"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ardf_cost.json"))
    args = ap.parse_args()
    import torch
    import helpers as H
    drv = H.GpuDriver()
    out = dict(rounds=args.rounds)
    h, typ, x = H.pbte_supercell((args.reps,) * 3, rattle=0.03, seed=17)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    in_process(drv, torch, H.golden("PbTe", "nep.txt"), h, typ, x, mass, args, out)
    if args.ref:
        binaries(args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("written: " + args.out)


if __name__ == "__main__":
    main()
