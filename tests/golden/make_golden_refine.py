"""Golden fixture of the REFINEMENT (text2protein_amd/refine.py, t2p_op_refine_backbone): the float64 oracle's runs on the chains of
fold_chains.npz under reproducible noise.

    python tests/golden/make_golden_refine.py

Nothing of the reference is read.  The cases, their noise and seeds are tests/refine_oracle.py's CASES; the maps are rebuilt from
fold_chains.npz by ``case_maps`` wherever they are needed, so only coordinates and scalars are written (refine_cases.npz).  Per case:
``start`` = fold_oracle.fold of the case's maps rounded to float32 (what the device's fold hands on), the oracle's coordinates, status,
iteration and evaluation counts after SHORT_ITERS iterations per stage, and after the default schedule its coordinates, energies, the
eight terms, counts, max|g|, closure, and the CA RMSD to the truth before and after.

The generator refuses a degenerate fixture: every run ends with status 0, the closure error ends under 0.01 A, and on every noisy case
the refined CA RMSD is below the fold's.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import fold_oracle as FO                                                # noqa: E402  (tests/)
import refine_oracle as RO                                              # noqa: E402  (tests/)

if __name__ == "__main__":
    gold = dict(np.load(os.path.join(HERE, "fold_chains.npz")))
    out, report = {}, {}
    for name in RO.CASES:
        maps = {k: v.astype(np.float64) for k, v in RO.case_maps(gold, name).items()}
        truth = RO.case_truth(gold, name)
        start = FO.fold(maps)["xyz"].astype(np.float32)
        x0 = start.astype(np.float64)
        short = RO.refine(x0, maps, RO.short_schedule(RO.SHORT_ITERS))
        full = RO.refine(x0, maps)
        before, after = FO.kabsch_rmsd(x0[:, 1], truth[:, 1]), FO.kabsch_rmsd(full["xyz"][:, 1], truth[:, 1])
        assert short["status"] == 0 and full["status"] == 0, (name, short["status"], full["status"])
        assert full["closure"] < 0.01 and full["e_end"] <= full["e_start"], (name, full["closure"])
        assert name not in RO.NOISY or after < before, (name, before, after)
        out[f"start_{name}"] = start
        out[f"short_xyz_{name}"] = short["xyz"]
        out[f"short_counts_{name}"] = np.array([short["status"], short["iterations"], short["evaluations"]])
        out[f"xyz_{name}"] = full["xyz"]
        out[f"terms_{name}"] = full["terms"]
        out[f"scalars_{name}"] = np.array([full["e_start"], full["e_end"], full["iterations"], full["evaluations"], full["gmax"], full["closure"],
                                           before, after])
        report[name] = dict(n=int(x0.shape[0]), noise=list(RO.CASES[name][1:3]), seed=RO.CASES[name][3], fold_ca_rmsd=before, refined_ca_rmsd=after,
                            fold_closure=FO.closure(x0), closure=full["closure"], e_start=full["e_start"], e_end=full["e_end"],
                            iterations=full["iterations"], evaluations=full["evaluations"], gmax=full["gmax"],
                            short=[short["iterations"], short["evaluations"]])
        print(name, json.dumps(report[name]), flush=True)
    out["meta"] = np.array(json.dumps(dict(cases=report, scalars=["e_start", "e_end", "iterations", "evaluations", "gmax", "closure",
                                                                  "fold_ca_rmsd", "refined_ca_rmsd"], short_iters=RO.SHORT_ITERS)))
    path = os.path.join(HERE, "refine_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote refine_cases.npz,", os.path.getsize(path), "bytes")
