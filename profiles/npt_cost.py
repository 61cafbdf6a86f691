#!/usr/bin/env python3
"""What a changing box costs: PbTe, 1,024,000 atoms (the 250-atom cell 16 x 16 x 16, triclinic), 300 K, 1 fs, six pressure
components (targets 0, modulus 40 GPa, tau_p 1000), on one engine per variant, alternating rounds in one process.

  (a) nepmi_run_npt_ber ms/step against nepmi_run_nvt_ber of the same library (what the per-step look at the device, the host
      re-metric and the barostat pass cost on top of the thermostat loop), and the list rebuilds per 100 steps of each;
  (b) the per-call sequence a drop-in host runs under one of its own NPT ensembles -- vv_step1, force_compute with the box of the
      step, vv_step2, find_thermo, berendsen_scale, berendsen_pressure -- with "keep_lists_on_box_change" off and on.

Host clock around calls that end in a device synchronise; one warm-up round per variant; measured, not asserted.

    python profiles/npt_cost.py [--reps 16] [--steps 100] [--rounds 3] [--out bench_out/npt_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GPA = 1.602177e+2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--emu", action="store_true", help="rehearsal on the kernel emulator (no timings worth reading)")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "npt_cost.json"))
    args = ap.parse_args()
    import helpers as H
    drv = H.EmuDriver() if args.emu else H.GpuDriver()
    nep = H.golden("PbTe", "nep.txt")
    h, typ, x = H.pbte_supercell((args.reps,) * 3, rattle=0.03, seed=17)
    h = np.array(h, dtype=np.float64).reshape(9)
    n = len(typ)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    vel = H.maxwell_velocities(mass, 300.0, seed=4)
    dt = 1.0 / H.TIME_UNIT
    p0, pc = np.zeros(6), np.full(6, GPA / (3.0 * 1000.0 * 40.0))
    model = drv.model(nep)

    def fresh(keep=None):
        eng = drv.engine(model, n)
        if keep is not None:
            eng.set_option("keep_lists_on_box_change", 1 if keep else 0)
        st = dict(t=drv.dev(typ), m=drv.dev(mass), x=drv.dev(x), v=drv.dev(vel), pe=drv.zeros(n), f=drv.zeros(3 * n), w=drv.zeros(9 * n),
                  th=drv.zeros(8), box=h.copy())
        eng.force_compute(st["box"], st["t"], st["x"], st["pe"], st["f"], st["w"])
        return eng, st

    def loop(kind):
        def run(eng, st, steps):
            a = (st["x"], st["v"], st["pe"], st["f"], st["w"])
            if kind == "npt_ber":
                eng.run_npt_ber(st["box"], st["t"], st["m"], dt, steps, 300.0, 300.0, 100.0, p0, pc, *a, thermo_every=steps)
            else:
                eng.run_nvt_ber(st["box"], st["t"], st["m"], dt, steps, 300.0, 300.0, 100.0, *a, thermo_every=steps)
        return run

    def stepwise(eng, st, steps):
        for _ in range(steps):
            eng.vv_step1(dt, st["m"], st["f"], st["x"], st["v"])
            eng.force_compute(st["box"], st["t"], st["x"], st["pe"], st["f"], st["w"])
            eng.vv_step2(dt, st["m"], st["f"], st["v"])
            vol = abs(np.linalg.det(st["box"].reshape(3, 3)))
            eng.find_thermo(vol, st["m"], st["pe"], st["v"], st["w"], st["th"])
            eng._ck(eng.lib.nepmi_berendsen_scale(eng.handle, n, 300.0, 1.0 / 100.0, eng._ptr(st["th"]), eng._ptr(st["v"])))
            eng.berendsen_pressure(st["box"], p0, pc, st["th"], st["x"])

    variants = {"run_nvt_ber": (fresh(), loop("nvt_ber")), "run_npt_ber": (fresh(), loop("npt_ber")),
                "per_call_keep_lists_off": (fresh(False), stepwise), "per_call_keep_lists_on": (fresh(True), stepwise)}
    res = {k: dict(ms_per_step=[], rebuilds_per_100_steps=[]) for k in variants}
    for rnd in range(args.rounds + 1):  # round 0 warms up
        for name, ((eng, st), fn) in variants.items():
            r0 = eng.stats().num_rebuild
            drv.sync()
            t0 = time.perf_counter()
            fn(eng, st, args.steps)
            drv.sync()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            if rnd > 0:
                res[name]["ms_per_step"].append(ms)
                res[name]["rebuilds_per_100_steps"].append((eng.stats().num_rebuild - r0) * 100.0 / args.steps)
    for name, ((eng, st), _) in variants.items():
        res[name]["describe"] = eng.describe()
        res[name]["median_ms_per_step"] = float(np.median(res[name]["ms_per_step"]))
    out = dict(atoms=n, steps_per_round=args.steps, rounds=args.rounds, results=res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    for name, r in res.items():
        print("%-26s %8.3f ms/step (rounds: %s), list rebuilds per 100 steps %s"
              % (name, r["median_ms_per_step"], " ".join("%.3f" % v for v in r["ms_per_step"]), r["rebuilds_per_100_steps"]))


if __name__ == "__main__":
    main()
