"""Classifier-free guidance in the predictor-corrector sampler, host side: the CPU restatement of a guided run (tests/guided_oracle.py)
against the reference fixtures, the C ABI's declarations, the score function's wrapper, the command line's refusal.  No GPU."""
import os
import re
import subprocess
import sys

import pytest
import torch

import guided_oracle as GO
from helpers import load_golden, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(GO.CASES))
def test_guided_oracle_reproduces_the_fixture(name):
    """The oracle's PC loop under the guidance expression, on the stored draws, against the reference's guided run: final sample and
    the state after every step within 1e-5; the same loop unguided lands on the stored unguided run and away from the guided one."""
    from text2protein_amd import synth
    case, g, steps = GO.CASES[name], load_golden(name), load_golden(name + "_steps")
    cfg = GO.case_config(case)
    shape = (GO.B, cfg.data.num_channels, cfg.data.max_res_num, cfg.data.max_res_num)
    sd = synth.synth_state_dict(cfg, GO.SEED)
    ctx = torch.from_numpy(g["context"])
    N, per = cfg.model.num_scales, case["n_steps_each"] + 1
    assert g["noise"].shape == (1 + N * per, *shape) and float(g["w"]) == case["w"] and int(g["nfe"]) == N * per
    assert float(g["difference"]) >= 20 * GO.F32_TOL[case["sde"]] and float(g["sensitivity"]) <= 10
    trace = []
    got, nfe = GO.guided_pc_run(sd, cfg, shape, ctx, case["w"], condition=GO.case_condition(case, shape[-1]), noise_fn=GO.replay(g["noise"]),
                                trace=trace)
    assert nfe == int(g["nfe"]) and len(trace) == N
    e = rel_l2(got, g["sample"])
    e_steps = max(max(rel_l2(x, steps["x"][i]), rel_l2(xm, steps["x_mean"][i])) for i, (x, xm) in enumerate(trace))
    plain, _ = GO.guided_pc_run(sd, cfg, shape, ctx, None, condition=GO.case_condition(case, shape[-1]), noise_fn=GO.replay(g["noise"]))
    print(f"{name}: guided oracle vs reference {e:.2e}, worst step {e_steps:.2e}; unguided oracle vs the guided reference "
          f"{rel_l2(plain, g['sample']):.2e}")
    assert e < 1e-5 and e_steps < 1e-5
    assert rel_l2(plain, g["unguided"]) < 1e-5 and rel_l2(plain, g["sample"]) > 20 * GO.F32_TOL[case["sde"]] / 2
    from oracle import t2p_oracle as O
    assert O.unet_forward.__module__ == "oracle.t2p_oracle"          # the wrapper is gone after the run


def test_new_symbols_are_declared_and_exported():
    from text2protein_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "t2p.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym, nargs in (("t2p_sampler_set_guidance", 3), ("t2p_sampler_set_context", 5), ("t2p_op_guided_langevin_norms", 11),
                       ("t2p_op_guided_langevin_update", 18), ("t2p_op_guided_predictor", 17)):
        m = re.search(r"\bint\s+" + sym + r"\s*\(([^)]*)\)\s*;", code)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs, sym
        assert sym in _lib.SIGNATURES and len(_lib.SIGNATURES[sym][1]) == nargs, sym
        assert hasattr(_lib.load(), sym)
    assert "diffusion_sampler.py:128" in hdr and "room for 2B samples" in hdr
    # the entry points that were there keep their signatures
    for sym, nargs in (("t2p_sampler_step", 6), ("t2p_sampler_step_graph", 4), ("t2p_sampler_run", 6), ("t2p_sampler_count_dispatches", 5),
                       ("t2p_op_langevin_update", 13), ("t2p_op_predictor", 11), ("t2p_ddim_set_context", 5)):
        m = re.search(r"\bint\s+" + sym + r"\s*\(([^)]*)\)\s*;", code)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[sym][1]), sym


class Stub:
    """Stands in for the network: records its calls, returns (1 + sum |context|) x."""

    def __init__(self):
        self.calls = []

    def eval(self):
        return self

    def __call__(self, x, labels, context):
        self.calls.append((x.clone(), labels.clone(), context.clone()))
        return x * (1.0 + context.abs().sum())


@pytest.mark.parametrize("kind", ["vesde", "vpsde"])
def test_score_fn_wrapper_issues_two_calls_with_the_zero_context_second(kind):
    from text2protein_amd import sampling, sde_lib
    from text2protein_amd._lib import T2PError
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=100.0, N=40) if kind == "vesde" else sde_lib.VPSDE(beta_min=0.1, beta_max=20.0, N=40)
    x = torch.randn(2, 5, 4, 4, generator=torch.Generator().manual_seed(1))
    ctx = torch.randn(2, 3, 8, generator=torch.Generator().manual_seed(2))
    t = torch.full((2,), 0.5)
    plain = Stub()
    base = sampling.get_score_fn(sde, plain)(x, t, ctx)
    assert len(plain.calls) == 1
    zero = sampling.get_score_fn(sde, Stub())(x, t, ctx * 0)
    for w in (0.7, 3.0, -1.0, 1.0, 0.0):
        stub = Stub()
        got = sampling.get_score_fn(sde, stub, guidance_w=w)(x, t, ctx)
        assert len(stub.calls) == 2
        (x1, l1, c1), (x2, l2, c2) = stub.calls
        assert torch.equal(c1, ctx) and torch.equal(c2, ctx * 0) and c2.shape == ctx.shape
        assert torch.equal(x1, x) and torch.equal(x2, x) and torch.equal(l1, l2) and torch.equal(l1, plain.calls[0][1])
        # w out(ctx) + (1 - w) out(0) on the network OUTPUT; the score's own scale (VP: -1 / std) comes after and is linear
        assert rel_l2(got, w * base + (1 - w) * zero) < 1e-6
    assert torch.equal(sampling.get_score_fn(sde, Stub(), guidance_w=None)(x, t, ctx), base)
    with pytest.raises(T2PError, match="finite"):
        sampling.get_score_fn(sde, Stub(), guidance_w=float("nan"))
    with pytest.raises(T2PError, match="context"):
        sampling.get_score_fn(sde, Stub(), guidance_w=0.7)(x, t, None)


def test_public_surface_takes_the_guidance_weight():
    import inspect
    from text2protein_amd import sampling
    for fn in (sampling.get_pc_sampler, sampling.get_score_fn, sampling.PCStepper.__init__, sampling.shared_predictor_update_fn,
               sampling.shared_corrector_update_fn):
        p = inspect.signature(fn).parameters["guidance_w"]
        assert p.default is None, fn
    assert hasattr(sampling.PCStepper, "set_context") and hasattr(sampling.PCStepper, "set_guidance")
    assert list(inspect.signature(sampling.get_score_fn).parameters) == ["sde", "model", "train", "continuous", "guidance_w"]


def test_cli_refuses_pc_guidance_with_ddim_before_touching_a_device():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for extra, word in ((["--sampler", "ddim", "--pc_guidance_w", "0.7"], "--sampler ddim"), (["--pc_guidance_w", "nan"], "finite")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "sampling_6d.py"), "no_such_config.yml", "synthetic", *extra],
                           capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode != 0 and "--pc_guidance_w" in r.stderr and word in r.stderr and "Traceback" not in r.stderr, r.stderr
