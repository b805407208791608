#!/usr/bin/env python3
"""ms per refinement in rounds (text2protein_amd/refine.py refine_rounds_batch) for 32 chains at L = 128 on the noisy maps
of tools/bench_refine.py, and what the rounds buy on the committed noisy cases.

    python tools/bench_refine_rounds.py [--runs 5] [--out profiles/refine_rounds_cond_length.json]
                                        [--parity_out profiles/refine_rounds_parity.json]

Time (--out).  The chains, the noise (1.0 A / 0.1 rad, torch seed 20240) and the start (the device's fold of the noisy maps) are those
of bench_refine.py's ``refine_noisy``.  Timed between device events, median of --runs calls after one untimed call, all in one process:
``refine_backbone_batch`` (the single minimisation), then ``refine_rounds_batch`` at rounds x replicas = 1 x 1, 5 x 1 and 5 x 8.  The
ratio of 5 x 8 to 5 x 1 is the claim that the extra candidates ride on idle compute units: 32 workgroups against 256 on 256 CUs.  The
parts of one round at 8 replicas are timed through the public operators the loop is made of -- ``perturb_torsions`` on 32 chains,
``refine_backbone_batch`` and ``restraint_energy`` on the 256 candidates it wrote (the same candidates the 1 x 8 call makes), with
the second round's schedule -- and the selection is what remains of the 1 x 8 call.  A call lasts as long as its slowest chain, so
the evaluation counts of the slowest candidate per round are recorded next to the times.

Quality (--parity_out).  Every noisy case of tests/refine_oracle.py (its recorded start) and the 48-residue chain under 2.0 A / 0.3 rad
(noisy_maps seed 21, started from the device's fold): E_sel of the kept chain and its CA RMSD to the truth after 1 and after 5 rounds
at 1 and at 8 replicas, next to the single minimisation.  No pass mark.  Lower E_sel is what the protocol guarantees, a lower RMSD is
not.  Maps sampled from a trained checkpoint are not measured: none exists in this repository.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NAMES = ("dist", "omega", "theta", "phi")


def ca_rmsd(got, truth):
    p, q = got - got.mean(0), truth - truth.mean(0)
    u, s, vt = np.linalg.svd(p.T @ q)
    s[-1] *= np.sign(np.linalg.det(u @ vt))
    return float(np.sqrt(max((p * p).sum() + (q * q).sum() - 2 * s.sum(), 0.0) / p.shape[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default="")
    ap.add_argument("--parity_out", default="")
    args = ap.parse_args()

    from text2protein_amd import refine as R
    from text2protein_amd.decode import decode_6d_batch
    from text2protein_amd.encode import encode_6d_batch
    from text2protein_amd.fold import fold_maps_batch

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B, L = args.batch, 128
    gold = np.load(os.path.join(ROOT, "tests", "golden", "fold_chains.npz"))
    truth = gold["xyz_132"][:L]
    xyz = torch.from_numpy(truth).float().unsqueeze(0).repeat(B, 1, 1, 1).to(dev)
    samples = encode_6d_batch(xyz, torch.full((B,), L, dtype=torch.int32))["coords_6d"]
    lengths, _, absval = decode_6d_batch(samples)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    med = statistics.median

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.runs):
            ev0.record()
            out = fn()
            ev1.record()
            torch.cuda.synchronize()
            ms.append(ev0.elapsed_time(ev1))
        return ms, out

    g = torch.Generator(device="cpu").manual_seed(20240)            # bench_refine.py's noisy maps
    z = torch.randn(B, 4, L, L, generator=g).to(dev)
    m = absval.reshape(B, 4, L, L)
    known = (m[:, 0] > 0) & (m[:, 0] < 20.0)
    noisy = m.clone()
    noisy[:, 0] = torch.where(known, (m[:, 0] + 1.0 * z[:, 0]).clamp(0.5, 19.99), m[:, 0])
    for c in (1, 2):
        a = m[:, c] + 0.1 * z[:, c]
        noisy[:, c] = torch.where(known, a - 2 * np.pi * torch.round(a / (2 * np.pi)), m[:, c])
    noisy[:, 3] = torch.where(known, (m[:, 3] + 0.1 * z[:, 3]).clamp(0.01, np.pi - 0.01), m[:, 3])
    noisy = noisy.reshape(B, 4, L * L).contiguous()
    start = fold_maps_batch(noisy, lengths)[0]
    rm = lambda x, b: ca_rmsd(x[b, :, 1].cpu().numpy().astype(np.float64), truth[:, 1])

    single_ms, single = timed(lambda: R.refine_backbone_batch(start, noisy, lengths))
    rows = {}
    for rounds, K in ((1, 1), (5, 1), (5, 8)):
        ms, (x, status, diag, trace) = timed(lambda: R.refine_rounds_batch(start, noisy, lengths, rounds, K))
        tr = trace.cpu().numpy()
        rows[f"{rounds}x{K}"] = {"ms": round(med(ms), 4), "ms_runs": [round(v, 4) for v in ms], "status": sorted(set(status.cpu().tolist())),
                                 "kept_per_round": (tr[..., 3].sum(axis=2) > 0).sum(axis=0).astype(int).tolist(),
                                 "evaluations_max_per_round": tr[..., 2].max(axis=(0, 2)).astype(int).tolist(),
                                 "ca_rmsd_mean": round(float(np.mean([rm(x, b) for b in range(B)])), 4),
                                 "bit_equal_to_single": bool(torch.equal(x, single[0])), "finite": bool(torch.isfinite(x).all())}
    # the parts of one round at 8 replicas under the second round's schedule, from the single minimisation's result
    K = 8
    sched = R.reference_rounds(2)[1]
    move_ms, (cand, _) = timed(lambda: R.perturb_torsions(single[0], lengths, replicas=K, stream=R.STREAM_STRIDE, keep_first=True))
    flat, maps_k, n_k = cand.reshape(B * K, L, 3, 3), noisy.repeat_interleave(K, 0), lengths.repeat_interleave(K)
    min_ms, (rx, _, _) = timed(lambda: R.refine_backbone_batch(flat, maps_k, n_k, sched))
    min1_ms, _ = timed(lambda: R.refine_backbone_batch(cand[:, 1].contiguous(), noisy, lengths, sched))
    energy_ms, _ = timed(lambda: R.restraint_energy(rx, maps_k, n_k, R.SELECT_STAGE))
    round_ms, (_, _, _, rtrace) = timed(lambda: R.refine_rounds_batch(single[0], noisy, lengths, 1, K, schedules=[sched],
                                                                      stream_base=R.STREAM_STRIDE))
    ev = rtrace.cpu().numpy()[:, 0, :, 2]
    parts = {"replicas": K, "move_ms": round(med(move_ms), 4), "minimise_256_workgroups_ms": round(med(min_ms), 4),
             "minimise_32_workgroups_ms": round(med(min1_ms), 4), "energy_ms": round(med(energy_ms), 4), "round_ms": round(med(round_ms), 4),
             "evaluations_max_256": int(ev.max()), "evaluations_max_32": int(ev[:, 1].max()),
             "us_per_evaluation_256": round(1e3 * med(min_ms) / ev.max(), 3), "us_per_evaluation_32": round(1e3 * med(min1_ms) / ev[:, 1].max(), 3)}
    parts["selection_and_rest_ms"] = round(parts["round_ms"] - parts["move_ms"] - parts["minimise_256_workgroups_ms"] - parts["energy_ms"], 4)
    parts["move_share_of_round"] = round(parts["move_ms"] / parts["round_ms"], 5)
    out = {"what": "ms per refinement in rounds (32 chains, L = 128, noisy maps of bench_refine.py, reference schedules), same process",
           "L": L, "chains": B, "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "refine_backbone_ms": round(med(single_ms), 4), "refine_backbone_ms_runs": [round(v, 4) for v in single_ms],
           "rounds_x_replicas": rows, "ratio_5x8_over_5x1": round(rows["5x8"]["ms"] / rows["5x1"]["ms"], 4),
           "ratio_5x8_over_5x1_slowest_chain_evaluations": round(sum(rows["5x8"]["evaluations_max_per_round"]) /
                                                                 sum(rows["5x1"]["evaluations_max_per_round"]), 4),
           "ratio_1x1_over_refine_backbone": round(rows["1x1"]["ms"] / med(single_ms), 4), "one_round_parts": parts,
           "start_ca_rmsd_mean": round(float(np.mean([rm(start, b) for b in range(B)])), 4),
           "refine_backbone_ca_rmsd_mean": round(float(np.mean([rm(single[0], b) for b in range(B)])), 4)}
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    if args.parity_out:
        import refine_oracle as RO
        cases = np.load(os.path.join(ROOT, "tests", "golden", "refine_cases.npz"))
        todo = [(name, RO.case_maps(gold, name), cases[f"start_{name}"], RO.case_truth(gold, name), list(RO.CASES[name][1:3])) for name in RO.NOISY]
        clean48 = {k: gold[f"{k}_48"] for k in NAMES}
        todo.append(("48 at 2.0 A / 0.3 rad", RO.noisy_maps(clean48, 2.0, 0.3, 21), None, gold["xyz_48"], [2.0, 0.3]))
        report = {}
        for name, maps, x0, tr_xyz, noise in todo:
            n = maps["dist"].shape[0]
            a = torch.stack([torch.from_numpy(maps[k].reshape(-1)) for k in NAMES]).unsqueeze(0).to(dev).contiguous()
            n_t = torch.tensor([n], dtype=torch.int32)
            x = fold_maps_batch(a, n_t)[0] if x0 is None else torch.from_numpy(x0).unsqueeze(0).to(dev)
            rmsd = lambda t: round(ca_rmsd(t[0, :, 1].cpu().numpy().astype(np.float64), tr_xyz[:, 1].astype(np.float64)), 4)
            sx, sst, _ = R.refine_backbone_batch(x, a, n_t)
            row = {"residues": n, "noise": noise, "start": "device fold" if x0 is None else "recorded fold", "start_ca_rmsd": rmsd(x),
                   "single": {"status": int(sst[0]), "e_sel": float(R.restraint_energy(sx, a, n_t, R.SELECT_STAGE)[0][0, 8]), "ca_rmsd": rmsd(sx)}}
            for rounds in (1, 5):
                for K in (1, 8):
                    rx, rst, _, trace = R.refine_rounds_batch(x, a, n_t, rounds, K)
                    t = trace.cpu().numpy()[0]
                    row[f"{rounds}x{K}"] = {"status": int(rst[0]), "e_sel": float(t[..., 0][t[..., 3] > 0].min()), "ca_rmsd": rmsd(rx),
                                            "kept": [int(np.nonzero(t[r, :, 3])[0][0]) if t[r, :, 3].any() else None for r in range(rounds)],
                                            "candidate_status": sorted(set(t[..., 1].astype(int).reshape(-1).tolist()))}
            report[name] = row
            print(name, json.dumps(row), flush=True)
        doc = {"what": "E_sel (SELECT_STAGE total of the kept chain) and CA RMSD to the truth after 1 and 5 rounds at 1 and 8 replicas, "
                       "next to the single minimisation; seed 0, amplitude 10 degrees, reference schedules",
               "device": torch.cuda.get_device_name(0), "cases": report,
               "cpu_prototype": {"48 at 2.0 A / 0.3 rad": {"single": {"e_sel": 2341.47, "ca_rmsd": 0.971}, "5x2": {"e_sel": 2326.31, "ca_rmsd": 0.829}},
                                 "48 at 3.0 A / 0.4 rad": {"single": {"e_sel": 6514, "ca_rmsd": 2.20}, "5x2": {"e_sel": 5715, "ca_rmsd": 2.73},
                                                           "note": "every run ended with status 1; the energy improved, the RMSD did not"}},
               "not_measured": "maps sampled from a trained checkpoint (none exists in this repository)"}
        with open(args.parity_out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
