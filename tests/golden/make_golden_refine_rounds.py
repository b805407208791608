"""Golden fixture of the REFINEMENT IN ROUNDS (text2protein_amd/refine.py refine_rounds_batch, t2p_op_refine_rounds): the float64
oracle's run of the protocol (tests/refine_rounds_oracle.py) on two chains of refine_cases.npz.

    python tests/golden/make_golden_refine_rounds.py

Nothing of the reference is read.  The run is ``refine_rounds_oracle.PROTOCOL``: chains 96w8 and 96cut from their recorded starts, two
rounds of three candidates, the short schedule per round with the round's weights.  Per chain the fixture holds the kept candidate of
every round, every candidate's E_sel, status and evaluation count, and the final coordinates (refine_rounds.npz).

A selection between two nearly equal energies could go either way on another machine, so seeds are searched from 0 up until, for
every chain and round, the two lowest E_sel among the candidates and the incumbent differ by at least MIN_GAP (relative); the seed
found is stored.  The generator also refuses a run in which no perturbed candidate is ever kept: it would not test the selection.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import refine_oracle as RO                                              # noqa: E402  (tests/)
import refine_rounds_oracle as RR                                       # noqa: E402  (tests/)


def run(seed, fold_gold, cases):
    P = RR.PROTOCOL
    schedules = [RR.round_schedule(r, P["iters"]) for r in range(P["rounds"])]
    return [RR.rounds(cases[f"start_{name}"], RO.case_maps(fold_gold, name), schedules, RR.SELECT_STAGE, P["replicas"], P["amp"], seed,
                      P["stream_base"], cid) for name, cid in zip(P["chains"], P["chain_ids"])]


if __name__ == "__main__":
    fold_gold = dict(np.load(os.path.join(HERE, "fold_chains.npz")))
    cases = dict(np.load(os.path.join(HERE, "refine_cases.npz")))
    for seed in range(64):
        res = run(seed, fold_gold, cases)
        gaps = np.array([RR.selection_gaps(r["esel"], r["cstatus"]) for r in res])
        moved = any(k > 0 for r in res for k in r["kept"])
        print(f"seed {seed}: smallest gap {gaps.min():.3e}, kept {[r['kept'] for r in res]}", flush=True)
        if gaps.min() >= RR.MIN_GAP and moved:
            break
    else:
        raise SystemExit("no seed below 64 gives every selection a margin")
    out = dict(seed=np.array(seed), kept=np.array([r["kept"] for r in res]), esel=np.stack([r["esel"] for r in res]),
               cstatus=np.stack([r["cstatus"] for r in res]), evals=np.stack([r["evals"] for r in res]),
               status=np.array([r["status"] for r in res]), gaps=gaps)
    for name, r in zip(RR.PROTOCOL["chains"], res):
        out[f"xyz_{name}"] = r["xyz"]
        out[f"diag_energy_{name}"] = np.array(r["run"]["e_end"])
    out["meta"] = np.array(json.dumps(dict(protocol=RR.PROTOCOL, min_gap=RR.MIN_GAP, select_stage=RR.SELECT_STAGE)))
    path = os.path.join(HERE, "refine_rounds.npz")
    np.savez_compressed(path, **out)
    print("wrote refine_rounds.npz,", os.path.getsize(path), "bytes")
