"""CPU-side checks: config surface, structure tables, synthetic data, host logic, and that the
C-ABI library loads and exports every symbol include/t2p.h declares (no compute without a GPU)."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import cfg_tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_configs_load_and_param_counts():
    from text2protein_amd.arch import build_arch, param_specs
    from text2protein_amd.config import load_config
    n = {}
    for name, over in [("test_config.yml", {"data.max_res_num": 128}), ("test_config.yml", {"data.max_res_num": 64}),
                       ("cond_length.yml", {}), ("test_config_large.yml", {}), ("cond_length_inpainting.yml", {})]:
        cfg = load_config(os.path.join(ROOT, "configs", name), **over)
        assert cfg.model.n_heads == 8 and cfg.model.context_dim == 4096    # defaults supplied
        specs = param_specs(cfg)
        n[(name, cfg.data.max_res_num)] = sum(int(np.prod(s.shape)) for s in specs)
        a = build_arch(cfg)
        assert len(a.input_stages) == len(cfg.model.ch_mult) * cfg.model.num_res_blocks + len(cfg.model.ch_mult) - 1
    # parameter counts probed from the reference model
    assert round(n[("test_config.yml", 128)] / 1e6, 1) == 379.5
    assert round(n[("test_config.yml", 64)] / 1e6, 1) == 345.4
    assert round(n[("cond_length.yml", 128)] / 1e6, 1) == 75.0
    assert round(n[("test_config_large.yml", 256)] / 1e6, 1) == 863.3


def test_attrdict_behaviour():
    from text2protein_amd.config import AttrDict, finalize_config
    c = AttrDict({"a": {"b": 1}, "l": [{"x": 2}]})
    assert c.a.b == 1 and c["a"]["b"] == 1 and c.l[0].x == 2
    c.a.b = 5
    assert c["a"]["b"] == 5
    with pytest.raises(AttributeError):
        c.missing
    cfg = finalize_config({"model": {"condition": None}, "data": {}}, **{"data.max_res_num": 7})
    assert cfg.model.condition == [] and cfg.data.max_res_num == 7 and cfg.model.n_heads == 8


def test_synth_is_deterministic_and_non_degenerate():
    from text2protein_amd import synth
    from text2protein_amd.arch import param_specs
    cfg = cfg_tiny()
    a = synth.synth_state_dict(cfg, 3)
    b = synth.synth_state_dict(cfg, 3)
    c = synth.synth_state_dict(cfg, 4)
    for s in param_specs(cfg):
        assert torch.equal(a[s.name], b[s.name])
        assert float(a[s.name].abs().max()) > 1e-4, s.name       # nothing zero / 1e-10 scaled
    assert not torch.equal(a["pre_conv.weight"], c["pre_conv.weight"])
    w = a["mid_blocks.0.Conv_0.weight"]
    assert abs(float(w.var()) * w[0].numel() - 1.0) < 0.15       # variance 1 / fan_in
    z = synth.normal(0, "z", 200000)
    assert abs(float(z.mean())) < 0.01 and abs(float(z.std()) - 1) < 0.01
    # chunked generation equals one-shot generation
    assert np.array_equal(synth.uniform_pm1(1, "t", 1000, chunk=64), synth.uniform_pm1(1, "t", 1000))


def test_condition_builders_match_oracle():
    from oracle import t2p_oracle as O
    from text2protein_amd import conditions
    cfg = cfg_tiny()
    m = conditions.get_mask_all_lengths(cfg, batch_size=3)
    assert torch.equal(m, O.mask_all_lengths(cfg.data.min_res_num, cfg.data.max_res_num, 3))
    cfg.model.condition = ["inpainting"]
    batch = conditions.selected_mask_batch({"coords_6d": torch.zeros(2, 5, 16, 16)}, "1:3,6,9:10", cfg)
    assert torch.equal(batch["mask_inpaint"], O.selected_mask("1:3,6,9:10", 2, 16))
    cfg.model.condition = []
    assert conditions.selected_mask_batch({"coords_6d": torch.zeros(2, 5, 16, 16)}, "1:3", cfg)["mask_inpaint"] is None


def test_apply_conditions_matches_oracle():
    from oracle import t2p_oracle as O
    from text2protein_amd import sampling
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 8, 16, 16, generator=g)
    cond = {"length": O.mask_all_lengths(4, 16, 2)[7], "ss": torch.randn(2, 3, 16, 16, generator=g),
            "inpainting": {"coords_6d": torch.rand(2, 8, 16, 16, generator=g), "mask_inpaint": O.selected_mask("1:5", 2, 16)}}
    a, am = sampling.apply_conditions(x.clone(), cond)
    b, bm = O.apply_conditions(x.clone(), cond)
    assert torch.equal(a, b) and torch.equal(am, bm)


def test_sde_tables_match_golden():
    """The product's tables are the reference's float32 arithmetic: bit for bit against the oracle's restatement on this host,
    and within float32 rounding of the reference's own tables (helpers.F32_HOST_RTOL)."""
    import torch
    from helpers import assert_table_close, load_golden, ve_g_rtol
    from oracle import t2p_oracle as O
    from text2protein_amd import sde_lib
    g = load_golden("tables")
    for N in (100, 1000, 2000):
        sde = sde_lib.VESDE(0.01, 100.0, N)
        dsig, ts = O.ve_discrete_sigmas(0.01, 100.0, N), O.timesteps(N, 1e-5)
        assert torch.equal(sde.discrete_sigmas, dsig)
        assert torch.equal(sde.g_table(1e-5), torch.cat([O.ve_discretize_G(ts[i:i + 1], dsig, N) for i in range(N)]))
        assert_table_close(sde.discrete_sigmas, g[f"discrete_sigmas_{N}"])
        assert_table_close(sde.g_table(1e-5), g[f"G_{N}"], ve_g_rtol(N))
        vp, ovp = sde_lib.VPSDE(0.1, 20.0, N), O.vp_tables(0.1, 20.0, N)
        assert torch.equal(vp.alphas, ovp["alphas"]) and torch.equal(vp.sqrt_1m_alphas_cumprod, ovp["sqrt_1m_alphas_cumprod"])
        assert_table_close(vp.alphas, g[f"vp_alphas_{N}"])
        assert_table_close(vp.sqrt_1m_alphas_cumprod, g[f"vp_sqrt_1m_acp_{N}"])


def test_registries_and_errors():
    from text2protein_amd import sampling, sde_lib
    assert sampling.get_predictor("reverse_diffusion") is sampling.ReverseDiffusionPredictor
    with pytest.raises(KeyError):
        sampling.get_predictor("euler_maruyama")
    with pytest.raises(ValueError):
        sampling.register_corrector(name="langevin")(sampling.LangevinCorrector)

    class Other:
        pass

    with pytest.raises(NotImplementedError):
        sampling.get_score_fn(Other(), lambda *a: None)
    with pytest.raises(NotImplementedError):
        sampling.LangevinCorrector(Other(), None, 0.1, 1)
    assert sde_lib.VESDE(0.01, 100, 10).T == 1


def test_c_abi_library_exports_every_declared_symbol():
    from text2protein_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "t2p.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(t2p_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name


def test_no_gpu_means_loud_failure():
    """Without a GPU the product path refuses to run: there is no CPU fallback."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import ctypes as C
    from text2protein_amd import _lib
    from text2protein_amd.model import HipScoreModel, _model_config
    lib = _lib.load()
    assert lib.t2p_device_count() <= 0
    h = C.c_void_p()
    mc = _model_config(cfg_tiny(), "f32")
    assert lib.t2p_engine_create(C.byref(mc), C.byref(h)) != 0
    assert b"no HIP device" in lib.t2p_last_error()
    with pytest.raises(Exception):
        HipScoreModel(cfg_tiny(), device="cuda:0")
    with pytest.raises(_lib.T2PError):
        HipScoreModel(cfg_tiny(), device="cpu")


def test_product_path_does_not_import_the_oracle():
    import ast
    pkg = os.path.join(ROOT, "text2protein_amd")
    for fn in list(os.listdir(pkg)) + ["../sampling_6d.py"]:
        if not fn.endswith(".py"):
            continue
        tree = ast.parse(open(os.path.join(pkg, fn)).read())
        for node in ast.walk(tree):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""]
            assert not any(n.split(".")[0] == "oracle" for n in names), fn


def test_checkpoint_roundtrip_layout(tmp_path):
    from text2protein_amd import checkpoint, synth
    cfg = cfg_tiny()
    p = checkpoint.save_synthetic_checkpoint(str(tmp_path / "ckpt.pth"), cfg, seed=2)
    st = torch.load(p, weights_only=False)
    assert set(st) == {"optimizer", "model", "ema", "step"}
    assert all(k.startswith("module.") for k in st["model"])
    assert st["model"]["module.sigmas"].dtype == torch.float64
    sd = checkpoint.ema_state_dict(cfg, st)
    ref = synth.synth_state_dict(cfg, 2)
    assert list(sd) == list(ref) and all(torch.equal(sd[k], ref[k]) for k in ref)
    assert checkpoint.strip_module_prefix(st["model"]).keys() >= ref.keys()


def test_build_flags_scratch_spills():
    """The build fails when an LDS-DMA GEMM kernel uses scratch memory (a rolled accumulator loop is
    correct but several times slower): the parser behind that check."""
    from text2protein_amd.build import scratch_users
    remarks = """gemm.hip:1:1: remark: Function Name: _ZN3t2p15gemm_dma_kernelIaEEv [-Rpass-analysis=kernel-resource-usage]
gemm.hip:1:1: remark:     VGPRs: 256 [-Rpass-analysis=kernel-resource-usage]
gemm.hip:1:1: remark:     ScratchSize [bytes/lane]: 544 [-Rpass-analysis=kernel-resource-usage]
gemm.hip:2:1: remark: Function Name: _ZN3t2p15gemm_dma_kernelIbEEv [-Rpass-analysis=kernel-resource-usage]
gemm.hip:2:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
gemm.hip:3:1: remark: Function Name: _ZN3t2p11gemm_kernelIfEEv [-Rpass-analysis=kernel-resource-usage]
gemm.hip:3:1: remark:     ScratchSize [bytes/lane]: 16 [-Rpass-analysis=kernel-resource-usage]"""
    assert scratch_users(remarks) == [("_ZN3t2p15gemm_dma_kernelIaEEv", 544), ("_ZN3t2p11gemm_kernelIfEEv", 16)]
    assert scratch_users(remarks, "gemm_dma_kernel") == [("_ZN3t2p15gemm_dma_kernelIaEEv", 544)]


def test_build_hashes_every_source_and_header():
    """Every file of csrc/ is in build.SOURCES or build.HEADERS and every listed file exists: a file left out of source_hash
    lets a stale library load."""
    from text2protein_amd import build
    listed = build.SOURCES + build.HEADERS
    assert len(set(listed)) == len(listed)
    for f in listed:
        assert os.path.isfile(os.path.join(build.CSRC, f)), f
    on_disk = {f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp", ".h"))}
    assert on_disk and on_disk <= set(listed), sorted(on_disk - set(listed))


def test_oracle_stands_on_its_own_topology():
    """The oracle derives the module sequence from the config itself (no import of the product package) and agrees with the
    product's arch table -- and so, through param_tables.json, with the reference's named_parameters() -- on every shipped YAML."""
    import re
    from oracle import t2p_oracle as O
    from text2protein_amd.arch import build_arch
    from text2protein_amd.config import load_config
    src = open(O.__file__).read()
    assert not re.search(r"^\s*(from|import)\s+text2protein_amd", src, re.M)
    for y, L in (("test_config.yml", 128), ("cond_length.yml", 128), ("cond_length_inpainting.yml", 128), ("test_config_large.yml", 256)):
        cfg = load_config(os.path.join(ROOT, "configs", y), **{"data.max_res_num": L})
        a = build_arch(cfg)
        mine = [[(l.kind, l.prefix, l.up, l.down) for l in st.layers] for st in a.input_stages + [a.mid_stage] + a.out_stages]
        ins, mid, outs = O.unet_plan(cfg)
        assert ins + [mid] + outs == mine


def test_condition_builders_match_the_loop_form():
    """get_mask_all_lengths / selected_mask_batch / get_condition_from_batch against the statement-by-statement form of
    reference utils.py:62-106,139-148 written out here."""
    import numpy as np
    import torch
    from text2protein_amd import conditions as Cn
    from text2protein_amd.config import tiny_config
    cfg = tiny_config(**{"data.min_res_num": 3, "data.max_res_num": 12, "model.condition": ["length", "inpainting"], "data.num_channels": 8})
    got = Cn.get_mask_all_lengths(cfg, batch_size=3)
    lengths = np.arange(3, 13)
    want = torch.zeros(len(lengths), 3, 12, 12).bool()
    for i, l in enumerate(lengths):
        want[i, :, :l, :l] = True
    assert got.dtype == torch.bool and torch.equal(got, want)
    for info in ("1:5,10:11", "0", "2,4:4,7:20", "3:-2"):
        m = torch.zeros(2, 12)
        for r in info.split(","):
            if ":" in r:
                a, b = r.split(":")
                m[:, int(a):int(b) + 1] = 1
            else:
                m[:, int(r)] = 1
        assert torch.equal(Cn.parse_mask_info(info, 2, 12), m)
        pair = torch.logical_or(m.unsqueeze(-1), m.unsqueeze(1)).bool()
        batch = Cn.selected_mask_batch({"coords_6d": torch.zeros(2, 8, 12, 12)}, info, cfg)
        assert torch.equal(batch["mask_inpaint"], pair)
    coords = torch.rand(2, 8, 12, 12) * 2 - 1
    c = Cn.get_condition_from_batch(cfg, {"coords_6d": coords, "aa_str": ["ACDEF_______", "ACDEFGHIK___"]}, mask_info="1:2,5")
    assert list(c) == ["length", "inpainting"]
    assert c["length"][0, :5, :5].all() and c["length"][0].sum() == 25 and c["length"][1].sum() == 81
    assert torch.equal(c["inpainting"]["coords_6d"], coords) and c["inpainting"]["mask_inpaint"][0, 1].all()
    assert not c["inpainting"]["mask_inpaint"][0, 0, 0]
    c2 = Cn.get_condition_from_batch(cfg, {"coords_6d": coords, "lengths": [5, 9]}, mask_info="1:2,5")
    assert torch.equal(c2["length"], c["length"])
    import pytest
    with pytest.raises(ValueError):
        Cn.get_condition_from_batch(cfg, {"coords_6d": coords, "lengths": [5, 9]})
    cfg_ss = tiny_config(**{"data.num_channels": 8, "model.condition": ["length", "ss"]})
    Lss = cfg_ss.data.max_res_num
    cs = torch.rand(1, 8, Lss, Lss)
    assert torch.equal(Cn.get_condition_from_batch(cfg_ss, {"coords_6d": cs, "lengths": [4]})["ss"], cs[:, 4:7])


def test_registries_raise_like_the_reference():
    """Duplicate name -> ValueError, unknown name -> KeyError (reference sampling.py:32-75); both decorator spellings."""
    import pytest
    from text2protein_amd import sampling as S
    assert S.get_predictor("reverse_diffusion") is S.ReverseDiffusionPredictor
    assert S.get_corrector("langevin") is S.LangevinCorrector
    with pytest.raises(KeyError):
        S.get_predictor("nope")
    with pytest.raises(KeyError):
        S.get_corrector("nope")
    with pytest.raises(ValueError, match="Already registered"):
        S.register_predictor(name="reverse_diffusion")(S.ReverseDiffusionPredictor)

    @S.register_corrector
    class _PlainNameCorrector(S.Corrector):
        def update_fn(self, x, t, context=None):
            return x, x
    try:
        assert S.get_corrector("_PlainNameCorrector") is _PlainNameCorrector
        with pytest.raises(ValueError):
            S.register_corrector(_PlainNameCorrector)
        with pytest.raises(TypeError):
            S.Predictor(None, None)                      # abstract
    finally:
        del S._CORRECTORS["_PlainNameCorrector"]


def test_checkpoint_loads_without_arbitrary_unpickling():
    """A reference-written checkpoint (tests/golden/tiny_checkpoint.pth) is plain tensors / containers: weights_only=True."""
    import torch
    from text2protein_amd import checkpoint as K
    src = open(K.__file__).read()
    assert "weights_only=True" in src and "weights_only=False" not in src
    d = torch.load(os.path.join(ROOT, "tests", "golden", "tiny_checkpoint.pth"), map_location="cpu", weights_only=True)
    assert set(d) == {"optimizer", "model", "ema", "step"} and len(d["ema"]["shadow_params"]) > 0


def test_cli_refuses_mask_info_without_a_source(tmp_path):
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sampling_6d.py"), os.path.join(ROOT, "configs", "cond_length_inpainting.yml"),
                        "synthetic", "--mask_info", "1:5"], capture_output=True, text=True)
    assert r.returncode != 0 and "--inpaint_coords" in (r.stderr + r.stdout)


def test_bench_line_carries_the_contract_keys():
    """Static check of bench.py: the keys the driver and the review read are all written (no GPU here)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    for key in ('"metric"', '"value"', '"unit"', '"n_gpus"', '"steps"', '"warmup"', '"ms_per_step"', '"higher_is_better"', '"scaling"',
                '"vs_baseline"', '"dtype"', '"data"', '"config"', '"workload"', '"roofline"', '"cpu_baseline"', '"bound"', '"achieved"',
                '"peak"', '"frac"', '"traffic"', '"cores"', '"kind"', '"sample"', '"dispatches_per_step"', '"traffic_measured_in_run"',
                '"f32"', '"cfg3"'):
        assert key in src, key
    assert 'out["roofline"]' in src and 'out["cpu_baseline"]' in src and "D.barrier(dist, dev)" in src and "D.max_over_ranks(" in src


def test_vp_tables_follow_the_reference_arithmetic():
    """sde_lib.VPSDE.vp_tables: the per-step tables of the fused VP loop restated from sde_lib.py:106-157, models/utils.py:138-157 and
    sampling.py:184-186 with plain loops."""
    import numpy as np
    import torch
    from text2protein_amd import sde_lib
    N, eps = 40, 1e-3
    sde = sde_lib.VPSDE(beta_min=0.1, beta_max=20.0, N=N)
    label_f, scale, xc, alpha = sde.vp_tables(eps)
    g = sde.g_table(eps)
    lab = sde.label_table(eps)
    ts = torch.linspace(1.0, eps, N)
    betas = torch.linspace(0.1 / N, 20.0 / N, N)
    alphas = 1.0 - betas
    s1m = torch.sqrt(1.0 - torch.cumprod(alphas, 0))
    for i in range(N):
        t = ts[i]
        k = int((t * (N - 1)).long())
        assert int(lab[i]) == k and float(label_f[i]) == float(t * (N - 1))
        assert float(scale[i]) == float(-1.0 / s1m[k])
        assert abs(float(xc[i]) - float(1.0 - (torch.sqrt(alphas[k]) - 1.0))) < 1e-7
        assert float(alpha[i]) == float(alphas[k]) and float(g[i]) == float(torch.sqrt(betas[k]))


def test_structure_workspace_sizes_are_pinned():
    """t2p_op_fold_ws / t2p_op_refine_ws / t2p_op_refine_rounds_ws are pure host functions over one 256-byte carve (WorkspaceCarve): a
    handful of their values, recorded from the library before the three workspace structs shared that carve, refusals included."""
    from text2protein_amd import _lib
    lib = _lib.load()
    assert [lib.t2p_op_fold_ws(*a) for a in ((1, 1), (3, 129), (32, 512), (1, 513), (0, 5))] == [1280, 261120, 36111360, -1, -1]
    assert [lib.t2p_op_refine_ws(*a) for a in ((1, 1), (3, 129), (32, 256), (1, 512), (0, 5))] == [1792, 2032896, 76316928, -1, -1]
    got = [lib.t2p_op_refine_rounds_ws(*a) for a in ((1, 5, 1, 1), (3, 129, 5, 8), (32, 256, 1, 8), (3, 128, 1, 17), (1, 512, 1, 1))]
    assert got == [8960, 16489472, 615307520, -1, -1]
