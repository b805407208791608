#!/usr/bin/env python3
"""Time of a weight refresh of the sampling engine from a trainer on the same GPU, next to the host route it replaces.

    python tools/bench_refresh.py [--out profiles/weight_refresh.json]

For configs/cond_length.yml (L = 128) and configs/test_config.yml (L = 64), f16 engine and trainer, synthetic weights:

  * device refresh -- ``HipScoreModel.load_from(trainer, "ema")`` on a loaded engine (in place), between device events, after one
    warm-up; the median of five with the spread (min, max);
  * host route     -- what the tree offered before: read the EMA to the host, create a new ``HipScoreModel``, ``load_ema_shadow``
    (which ends in the host ``finalize``); wall clock around a device synchronise, the median of three;
  * bandwidth floor -- the bytes the refresh reads and writes (counted by the engine while it packs) over 6.29 TB/s, the streaming
    rate measured for this GPU (8.0 TB/s by its data sheet), and the number of launches the refresh enqueues.

One JSON line on stdout (and in --out).  bench.py is not touched.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12
CASES = {"cond_length": ("cond_length.yml", 128), "test_config": ("test_config.yml", 64)}


def measure(name, yaml, L, dtype):
    from text2protein_amd import losses, synth
    from text2protein_amd._lib import check
    from text2protein_amd.config import load_config
    from text2protein_amd.model import HipScoreModel

    cfg = load_config(os.path.join(ROOT, "configs", yaml), **{"data.max_res_num": L, "model.num_scales": 1000})
    cfg.device = "cuda:0"
    W = synth.synth_state_dict(cfg, seed=0)
    n_params = sum(v.numel() for v in W.values())
    trainer = losses.HipTrainModel(cfg, device="cuda:0", dtype=dtype)
    trainer.load_state_dict(W)
    del W
    model = HipScoreModel(cfg, dtype=dtype, device="cuda:0")
    model.load_from(trainer, "ema")          # the first load allocates
    model.load_from(trainer, "ema")          # warm-up of the in-place refresh
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms, enqueue_ms = [], []
    for _ in range(5):
        ev0.record()
        t0 = time.perf_counter()
        model.load_from(trainer, "ema")
        enqueue_ms.append((time.perf_counter() - t0) * 1e3)
        ev1.record()
        torch.cuda.synchronize()
        dev_ms.append(ev0.elapsed_time(ev1))
    counts = (C.c_int64 * 3)()
    check(model.lib.t2p_engine_load_stats(model._h, counts))
    rd, wr, launches = (int(v) for v in counts)
    host_s = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        shadow = list(trainer.read(losses.EMA).values())
        fresh = HipScoreModel(cfg, dtype=dtype, device="cuda:0")
        fresh.load_ema_shadow(shadow)
        torch.cuda.synchronize()
        host_s.append(time.perf_counter() - t0)
        del fresh, shadow
    floor_ms = (rd + wr) / HBM_BYTES_PER_S * 1e3
    med = statistics.median(dev_ms)
    return {
        "config": name, "L": L, "dtype": dtype, "parameters": n_params,
        "device_refresh_ms": {"median": round(med, 3), "min": round(min(dev_ms), 3), "max": round(max(dev_ms), 3), "all": [round(v, 3) for v in dev_ms]},
        "device_refresh_enqueue_ms_median": round(statistics.median(enqueue_ms), 3),
        "host_route_s": {"median": round(statistics.median(host_s), 3), "all": [round(v, 3) for v in host_s]},
        "host_over_device": round(statistics.median(host_s) * 1e3 / med, 1),
        "bytes_read": rd, "bytes_written": wr, "launches": launches,
        "bandwidth_floor_ms": round(floor_ms, 4), "hbm_bytes_per_s": HBM_BYTES_PER_S,
        "refresh_over_floor": round(med / floor_ms, 1),
        "us_per_launch": round(med * 1e3 / max(launches, 1), 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f16", choices=["f32", "bf16", "f16"])
    ap.add_argument("--configs", default="cond_length,test_config")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_refresh needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    res = {"tool": "bench_refresh", "device": torch.cuda.get_device_name(0),
           "results": [measure(n, *CASES[n], args.dtype) for n in args.configs.split(",")]}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
