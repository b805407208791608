#!/usr/bin/env python3
"""6D backbone sampling on MI355X: the reference's ``sampling_6d.py`` command line on the HIP engine.

    python sampling_6d.py <config.yml> <checkpoint.pth> [--batch_size 32] [--tag test] [--device cuda]
                          [--select_length True --length_index 61] [--mask_info 1:5,10:15] [--n_iter 1]

Same positional arguments and flags as the reference (sampling_6d.py:41-53) and the same output
contract (one pickle per sample, tensor (1, C, L, L), under
sampling/coords_6d/<config stem>/<run>/<tag>/sampled_<id>.pkl, sampling_6d.py:160-162).
Differences, all at the edges of the hot path:
  * text context: the reference embeds captions with a LLaMA embedding table fetched by name
    (sampling_6d.py:121-137).  Here the same producer runs from local files: ``--captions <file>`` (one
    caption per line, optionally ``id<TAB>caption``) with ``--tokenizer_path <dir>`` and ``--embed_table
    <file or HF checkpoint dir>`` (only ``embed_tokens`` is read; the lookup is a HIP gather).  Without
    captions the context comes from ``--context <file.pt>`` (a (B, T, context_dim) float tensor) or is
    synthetic (``--context synthetic``).
  * ``--decode`` additionally writes ``decoded_<id>.npz`` per sample: the reference's first folding stage
    (sampling_rosetta.py:69-96: mask rounding, crop, clip, inverse scaling) done on the device.
  * ``--fold`` (implies ``--decode``) additionally folds every decoded sample to an N / CA / C backbone on the device
    (text2protein_amd/fold.py: restraint-free, in place of the PyRosetta stage of sampling_rosetta.py:98-160) and writes
    ``folded_<id>.pdb`` and ``fold_<id>.json`` (status, hand, closure errors, stress, restraint scores); one line is printed per
    chain whose status is not 0.
  * ``--refine`` (implies ``--fold``) additionally minimises every folded chain against the restraint set on the device
    (text2protein_amd/refine.py: a staged L-BFGS over the reference's restraints plus ideal-geometry terms, the step
    rosetta_min/run.py takes between the maps and TM-align -- without Rosetta's own energy terms, relax or side chains; maps of
    at most 256 residues) and writes ``refined_<id>.pdb`` next to ``folded_<id>.pdb``; ``fold_<id>.json`` gains a ``"refine"`` block
    (status, energies, the eight terms, iterations, evaluations, closure).  With ``--tm_ref`` the refined chains are the ones scored.
  * ``--refine_rounds R`` / ``--refine_replicas K`` (either implies ``--refine``; defaults 1 / 1 = the single minimisation above) run
    the minimisation in rounds as rosetta_min/run.py:88-151 does (text2protein_amd/refine.py ``refine_rounds_batch``): every round
    moves each phi and psi of the best chain so far by up to 10 degrees, K times, minimises the K candidates side by side with the
    round's weights and keeps the lowest-scoring one if it beats the best so far.  ``refined_<id>.pdb`` is the kept chain and the
    ``"refine"`` block gains ``"rounds"``: per round the candidates' E_sel, status and evaluations, and which was kept.  The draws
    are keyed by ``--seed``, the sample id and the ``--n_iter`` index.
  * ``--tm_ref PATH`` (repeatable; a ``.pdb`` file or a directory of them, read with ``--chain``; implies ``--fold``) scores the
    folded chains with TM-align on the device (text2protein_amd/tmalign.py, in place of the reference's one TMalign process per
    pair: tm/TMalign.py:36-160, utils.py:150-158): every chain against every reference and the chains against each other.
    ``tm_scores.json`` holds per sample min / max / avg / std over the references (normalised by the reference, as ``tm_score``
    does), the closest reference with both normalisations, and the pairwise matrix with its mean; one line is printed per sample.
  * ``--pdb FILE [--chain A] [--mask_info 1:5,10:15] [--sse LETTERS|FILE]``: the conditions of ``config.model.condition``
    from one chain of a PDB file (utils.py:122-137).  The reference goes through biotite there (and is broken, SURVEY.md 2
    row 10); here the backbone is read by a small reader of our own and featurised on the GPU (text2protein_amd/encode.py:
    dataset.py:114-168, :200-239, :396-450).  The secondary-structure letters of an 8-channel model (biotite's P-SEA in the
    reference) are an input: ``--sse`` takes one of a / b / c per residue, or a file holding them, or the word ``psea``: the
    letters are then computed from the chain's CA trace on the GPU (text2protein_amd/encode.py ``annotate_sse_batch``: P-SEA
    as DESIGN.md 8i states it).  Without ``--mask_info`` the reference's default "1:5,10:15" applies.
  * ``--ss_check`` (implies ``--fold``) annotates every folded chain the same way and adds an ``"sse"`` block to ``fold_<id>.json``:
    the letters and counts of the folded chain (and of the refined chain with ``--refine``) and, on an 8-channel model whose
    ``ss`` condition came from ``--pdb`` or ``--inpaint_coords``, the helix and strand agreement with the condition's own blocks
    (``encode.sse_target``); one line is printed per sample that has such a target.
  * ``--inpaint_coords <file.pt|synthetic>`` gives the same conditions from maps featurised elsewhere: built exactly as
    ``get_condition_from_batch`` does (utils.py:84-106).  ``--mask_info`` without either source is an error.
  * ``checkpoint`` may be the word ``synthetic`` (hash-generated weights, no file needed).
  * extra flags: --dtype (f32|f16|bf16), --seed, --ids, --num_scales / --max_res_num overrides.
  * ``--sampler ddim [--ddim_steps 50] [--ddim_eta 1.0] [--guidance_w 0.0]``: the reference's other sampler for the same network
    (sampler/diffusion_sampler.py: strided DDIM with classifier-free guidance on the text context) instead of the
    predictor-corrector loop.  It reads the network output as a noise prediction, so the config must say ``training.sde: vpsde``.
    The conditions and the output files are the same.
  * ``--pc_guidance_w W`` (with the default ``--sampler pc``, any config): the same guidance inside the predictor-corrector loop,
    every score made of ``W out(text) + (1 - W) out(no text)`` from one evaluation at twice the batch.  Unset is the plain loop.
  * ``--inpaint_mode replace`` (default ``condition``, today's behaviour): the residues ``--mask_info`` selects are designed and
    everything else of the chain given with ``--pdb`` / ``--inpaint_coords`` is held by *replacement* (the reference's
    score_sde_pytorch/inpainting.py: the known region is overwritten with the data noised to the current level after every
    update), which needs no ``inpainting`` condition in the config and so works with every checkpoint.  Not with ``--sampler ddim``.
Under ``python -m torch.distributed.run --nproc-per-node N`` (or with ``--gpus N``, which starts the N ranks
itself) every rank samples ``--batch_size`` chains on its own GPU and rank 0 gathers them with one RCCL
all_gather before writing (text2protein_amd/distributed.py).  ``--global_batch_norm`` reproduces the reference's
multi-GPU (DataParallel) Langevin step size: batch means over all ranks' chains, one 2-float all-reduce per step.
"""
import argparse
import os
import pickle as pkl
from pathlib import Path

import torch


def str2bool_like_reference(v):
    # the reference declares type=bool, so any non-empty string is True (sampling_6d.py:51)
    return bool(v)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("config", type=str)
    parser.add_argument("checkpoint", type=str)
    parser.add_argument("--pdb", type=str, default=None)
    parser.add_argument("--chain", type=str, default="A")
    parser.add_argument("--mask_info", type=str, default=None,
                        help="inpainting residue ranges (reference default '1:5,10:15'); needs --pdb or --inpaint_coords")
    parser.add_argument("--sse", type=str, default=None,
                        help="with --pdb and an 8-channel model: the chain's secondary-structure letters (one of a/b/c per residue), "
                             "a file holding them, or the word psea (computed from the CA trace on the GPU)")
    parser.add_argument("--tag", type=str, default="test")
    parser.add_argument("--device", type=str, default="cuda")
    parser.add_argument("--batch_size", type=int, default=32)
    parser.add_argument("--n_iter", type=int, default=1)
    parser.add_argument("--select_length", type=str2bool_like_reference, default=False)
    parser.add_argument("--length_index", type=int, default=1)  # Index starts at 1
    # additions
    parser.add_argument("--dtype", type=str, default="f16", choices=["f32", "f16", "bf16"])
    parser.add_argument("--context", type=str, default="synthetic")
    parser.add_argument("--context_tokens", type=int, default=512)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--ids", type=str, default=None, help="comma separated sample ids (default 0..B-1)")
    parser.add_argument("--num_scales", type=int, default=None)
    parser.add_argument("--max_res_num", type=int, default=None)
    parser.add_argument("--outdir", type=str, default=None)
    parser.add_argument("--captions", type=str, default=None, help="text file: one caption (or id<TAB>caption) per line")
    parser.add_argument("--tokenizer_path", type=str, default=None)
    parser.add_argument("--embed_table", type=str, default=None)
    parser.add_argument("--inpaint_coords", type=str, default=None,
                        help="source of the known 6D maps for the conditions of config.model.condition (what the reference "
                             "builds from --pdb, utils.py:84-137): a torch file holding {'coords_6d': (B or 1, C, L, L) in "
                             "[-1, 1], 'lengths': ints or 'aa_str': strings}, or the word 'synthetic' (U(-1, 1) maps, 100 residues)")
    parser.add_argument("--decode", action="store_true", help="also write decoded_<id>.npz (sampling_rosetta.py:69-96)")
    parser.add_argument("--fold", action="store_true",
                        help="also fold every decoded sample to an N / CA / C backbone on the GPU (text2protein_amd/fold.py; implies "
                             "--decode): folded_<id>.pdb and fold_<id>.json (status, hand, closure, stress, restraint scores)")
    parser.add_argument("--refine", action="store_true",
                        help="also minimise every folded chain against the restraint set on the GPU (text2protein_amd/refine.py; implies "
                             "--fold; at most 256 residues): refined_<id>.pdb next to folded_<id>.pdb, a \"refine\" block in fold_<id>.json; "
                             "--tm_ref then scores the refined chains")
    parser.add_argument("--refine_rounds", type=int, default=1, metavar="R",
                        help="minimise in R rounds (1..8; implies --refine): from the second round on every phi and psi of the best chain so "
                             "far moves by up to 10 degrees and the round's weights apply (rosetta_min/run.py); a result is kept only when it "
                             "scores lower; fold_<id>.json's \"refine\" block gains \"rounds\"")
    parser.add_argument("--refine_replicas", type=int, default=1, metavar="K",
                        help="candidates per round (1..16; implies --refine): K moves of the best chain so far are minimised side by side on "
                             "the GPU and the lowest-scoring one is the round's result")
    parser.add_argument("--ss_check", action="store_true",
                        help="also annotate the secondary structure of every folded (and refined) chain on the GPU (P-SEA; implies --fold): "
                             "an \"sse\" block in fold_<id>.json with the letters, the counts and, where the ss condition came from --pdb or "
                             "--inpaint_coords on an 8-channel model, the agreement with the condition's blocks")
    parser.add_argument("--tm_ref", type=str, action="append", default=None, metavar="PATH",
                        help="score every folded chain with TM-align on the GPU (text2protein_amd/tmalign.py) against reference chains: "
                             "PATH is a .pdb file or a directory of them, read with --chain; may be repeated; implies --fold; writes "
                             "tm_scores.json (per sample min / max / avg / std over the references, the closest one, and the pairwise "
                             "matrix of the samples)")
    parser.add_argument("--gpus", type=int, default=1, help="start this many ranks (one per GPU) when not under torch.distributed.run")
    parser.add_argument("--global_batch_norm", action="store_true",
                        help="Langevin batch means over every rank's chains (the reference's DataParallel semantics)")
    parser.add_argument("--sampler", type=str, default="pc", choices=["pc", "ddim"],
                        help="pc: the predictor-corrector SDE loop (default); ddim: strided DDIM with classifier-free guidance "
                             "(needs training.sde: vpsde)")
    parser.add_argument("--ddim_steps", type=int, default=50, help="--sampler ddim: loop steps (sampling_steps)")
    parser.add_argument("--ddim_eta", type=float, default=1.0, help="--sampler ddim: eta in [0, 1] (0 = deterministic)")
    parser.add_argument("--guidance_w", type=float, default=0.0,
                        help="--sampler ddim: eps = w eps(text) + (1 - w) eps(no text); the reference's default is 0")
    parser.add_argument("--pc_guidance_w", type=float, default=None,
                        help="--sampler pc: classifier-free guidance in the predictor-corrector loop, every score made of "
                             "w out(text) + (1 - w) out(no text) from one evaluation at twice the batch; 1 = the plain conditional "
                             "run; unset (default) = no guidance.  (--guidance_w belongs to --sampler ddim and defaults to 0, the "
                             "unconditional run)")
    parser.add_argument("--inpaint_mode", type=str, default="condition", choices=["condition", "replace"],
                        help="condition: the known maps enter as the config's `inpainting` condition (default); replace: replacement "
                             "inpainting in the predictor-corrector loop, for any checkpoint (needs --pdb or --inpaint_coords)")
    args = parser.parse_args()

    if args.pc_guidance_w is not None:                                  # before anything touches a device
        if args.sampler == "ddim":
            raise SystemExit("--pc_guidance_w guides the predictor-corrector loop: with --sampler ddim give --guidance_w")
        if args.pc_guidance_w != args.pc_guidance_w or args.pc_guidance_w in (float("inf"), float("-inf")):
            raise SystemExit("--pc_guidance_w must be finite")
    tm_ref_files = None
    if args.tm_ref is not None:                                         # host only: the paths are checked before anything touches a device
        from text2protein_amd.tmalign import reference_files
        try:
            tm_ref_files = reference_files(args.tm_ref)
        except ValueError as e:
            raise SystemExit(str(e))
        args.fold = True
    if not 1 <= args.refine_rounds <= 8 or not 1 <= args.refine_replicas <= 16:
        raise SystemExit("--refine_rounds takes 1..8 and --refine_replicas 1..16")
    in_rounds = args.refine_rounds > 1 or args.refine_replicas > 1
    if in_rounds:
        args.refine = True
    if args.refine or args.ss_check:
        args.fold = True
    replace = args.inpaint_mode == "replace"
    if replace:
        if args.sampler == "ddim":
            raise SystemExit("--inpaint_mode replace belongs to the predictor-corrector loop: not with --sampler ddim")
        if args.pdb is None and args.inpaint_coords is None:
            raise SystemExit("--inpaint_mode replace needs the known 6D maps: give --pdb <file> or --inpaint_coords <file.pt|synthetic>")
    assert not (args.pdb is not None and args.select_length)
    if args.pdb is not None and args.inpaint_coords is not None:
        raise SystemExit("--pdb and --inpaint_coords both name a source of the known 6D maps: give one")
    if args.sse is not None and args.pdb is None:
        raise SystemExit("--sse annotates the chain read with --pdb")
    if args.mask_info is not None and args.inpaint_coords is None and args.pdb is None:
        raise SystemExit("--mask_info selects residues of KNOWN 6D maps: give their source with --pdb <file> or --inpaint_coords <file.pt|synthetic>")
    assert not (args.inpaint_coords is not None and args.select_length)

    from text2protein_amd import distributed as D
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:      # before anything touches the GPU
        import sys
        raise SystemExit(D.launch_local(args.gpus, [os.path.abspath(__file__), *sys.argv[1:]]))
    from text2protein_amd import sampling, sde_lib, synth
    from text2protein_amd._lib import T2PError
    from text2protein_amd.checkpoint import restore_checkpoint
    from text2protein_amd.conditions import get_condition_from_batch, get_conditions_from_pdb, get_mask_all_lengths
    from text2protein_amd.config import load_config
    from text2protein_amd.model import HipScoreModel

    rank, world, local_rank = D.env_rank_world()
    overrides = {}
    if args.num_scales:
        overrides["model.num_scales"] = args.num_scales
    if args.max_res_num:
        overrides["data.max_res_num"] = args.max_res_num
    config = load_config(args.config, **overrides)
    if args.sampler == "ddim" and config.training.sde != "vpsde":      # before anything touches a device
        raise SystemExit(f"--sampler ddim needs a noise-prediction network: training.sde must be vpsde, {args.config} says "
                         f"{config.training.sde} (a VE-trained output is a score, not a noise prediction)")
    device = f"cuda:{local_rank}" if args.device == "cuda" else args.device
    config.device = device
    torch.cuda.set_device(torch.device(device))
    dist = D.init_process_group(device)

    run = Path(args.checkpoint).parent.parent.stem if args.checkpoint != "synthetic" else "synthetic"
    workdir = Path(args.outdir) if args.outdir else Path("sampling", "coords_6d", Path(args.config).stem, run, args.tag)
    if rank == 0:
        workdir.mkdir(parents=True, exist_ok=True)

    tm_refs = None
    if tm_ref_files is not None and rank == 0:                          # read once; a chain TM-align cannot take stops the run here
        from text2protein_amd import tmalign as TM
        try:
            tm_refs = TM.read_chains(tm_ref_files, args.chain) + ([os.path.basename(p) for p in tm_ref_files],)
        except ValueError as e:
            raise SystemExit(f"--tm_ref: {e}")
    # --ss_check: the target letters of the `ss` condition, one string per chain of this rank (the same on every rank)
    want_target = args.ss_check and config.data.num_channels == 8 and "ss" in config.model.condition
    ss_target = None
    pdb_condition = None
    if args.pdb is not None:
        sse = args.sse
        if sse is not None and sse != "psea" and os.path.exists(sse):
            sse = "".join(open(sse).read().split())
        try:
            # sampling_6d.py:146-147; the chain is the same for every iteration, so it is featurised once (and before the model is
            # built: a file that cannot be used is reported at once)
            pdb_condition = get_conditions_from_pdb(args.pdb, config, chain=args.chain, mask_info=args.mask_info or "1:5,10:15",
                                                    batch_size=args.batch_size, sse=sse, with_batch=replace or want_target)
        except (OSError, ValueError, T2PError) as e:
            raise SystemExit(f"--pdb: {e}")
        if want_target:
            from text2protein_amd.encode import sse_target
            ss_target = sse_target(pdb_condition["_batch"]["coords_6d"])
            if not replace:
                del pdb_condition["_batch"]

    # Initialize model (get_model + restore_checkpoint + ema.copy_to, sampling_6d.py:64-73)
    score_model = HipScoreModel(config, dtype=args.dtype, device=device)
    if args.checkpoint == "synthetic":
        score_model.load_state_dict(synth.synth_state_dict(config, args.seed))
    else:
        restore_checkpoint(args.checkpoint, score_model, config)

    # Load SDE (sampling_6d.py:76-82)
    if config.training.sde == "vesde":
        sde = sde_lib.VESDE(sigma_min=config.model.sigma_min, sigma_max=config.model.sigma_max, N=config.model.num_scales)
        sampling_eps = 1e-5
    elif config.training.sde == "vpsde":
        sde = sde_lib.VPSDE(beta_min=config.model.beta_min, beta_max=config.model.beta_max, N=config.model.num_scales)
        sampling_eps = 1e-3
    else:
        raise SystemExit(f"unknown training.sde {config.training.sde}")

    B = args.batch_size
    sampling_shape = (B, config.data.num_channels, config.data.max_res_num, config.data.max_res_num)
    kw = {}
    if args.global_batch_norm and dist is not None:
        kw = {"global_batch": B * world, "all_reduce": lambda sums: D.allreduce_norm_sums(sums, dist)}
    # every rank its own noise stream; every iteration of the --n_iter loop a fresh one (call index, sampling.py)
    if args.sampler == "ddim":
        from text2protein_amd.ddim import DiffusionSampler
        try:
            ddim = DiffusionSampler.from_sde(score_model, sde, sampling_steps=args.ddim_steps, ddim_eta=args.ddim_eta,
                                             w=args.guidance_w, seed=D.rank_seed(args.seed, rank))
        except T2PError as e:
            raise SystemExit(f"--sampler ddim: {e}")
        evaluations = args.ddim_steps * (1 if args.guidance_w == 1.0 else 2)

        def sampling_fn(model, condition=None, context=None):
            return ddim.ddim_sample(sampling_shape, context, condition=condition), evaluations
    elif replace:
        from text2protein_amd.inpainting import get_pc_inpainter, known_from_mask_info
        if args.pc_guidance_w is not None:
            kw["guidance_w"] = args.pc_guidance_w
        inpainter = get_pc_inpainter(sde, sampling.get_predictor(config.sampling.predictor.lower()),
                                     sampling.get_corrector(config.sampling.corrector.lower()), config.sampling.snr,
                                     n_steps=config.sampling.n_steps_each, probability_flow=config.sampling.probability_flow,
                                     denoise=config.sampling.noise_removal, eps=sampling_eps, seed=D.rank_seed(args.seed, rank), **kw)

        def sampling_fn(model, condition=None, context=None):
            # the maps are held by replacement, not by the `inpainting` condition; the other conditions apply as always
            batch = condition.pop("_batch")
            condition.pop("inpainting", None)
            data, known_mask = known_from_mask_info(config, batch, args.mask_info or "1:5,10:15", condition)
            return inpainter(model, data, known_mask, context=context, condition=condition)
    else:
        if args.pc_guidance_w is not None:
            kw["guidance_w"] = args.pc_guidance_w
        sampling_fn = sampling.get_sampling_fn(config, sde, sampling_shape, sampling_eps, seed=D.rank_seed(args.seed, rank), **kw)

    caption_ids = None
    if args.captions:
        if not (args.tokenizer_path and args.embed_table):
            raise SystemExit("--captions needs --tokenizer_path and --embed_table (local paths)")
        from text2protein_amd.text_context import TextContextProducer
        rows = [ln.rstrip("\n") for ln in open(args.captions) if ln.strip()]
        rows = rows[rank * B:(rank + 1) * B]
        if len(rows) != B:
            raise SystemExit(f"--captions must hold batch_size x world_size = {B * world} captions")
        if all("\t" in r for r in rows):
            caption_ids = [r.split("\t", 1)[0] for r in rows]
            rows = [r.split("\t", 1)[1] for r in rows]
        producer = TextContextProducer.from_local(args.tokenizer_path, args.embed_table, device=device)
        context = producer(rows)                           # sampling_6d.py:134-137
        if context.shape[-1] != config.model.context_dim:
            raise SystemExit(f"embedding width {context.shape[-1]} != model.context_dim {config.model.context_dim}")
        del producer
    elif args.context == "synthetic":
        context = synth.synth_context(B, args.context_tokens, config.model.context_dim, seed=D.rank_seed(args.seed, rank))
    else:
        context = torch.load(args.context, map_location="cpu")
        if context.shape[0] != B:
            raise SystemExit(f"context batch {context.shape[0]} != --batch_size {B}")
    ids = args.ids.split(",") if args.ids else (caption_ids or [str(rank * B + i) for i in range(B)])
    if len(ids) != B:
        raise SystemExit("--ids must list batch_size ids")

    known = None
    if args.inpaint_coords is not None:
        # the tensor half of get_conditions_from_pdb (utils.py:119-137): one featurised chain repeated over the batch
        C_, L_ = config.data.num_channels, config.data.max_res_num
        if args.inpaint_coords == "synthetic":
            coords = torch.from_numpy(synth.uniform_pm1(args.seed, "coords_6d", C_ * L_ * L_).reshape(1, C_, L_, L_))
            known = {"coords_6d": coords, "lengths": [min(100, L_)]}
        else:
            known = torch.load(args.inpaint_coords, map_location="cpu", weights_only=True)
            if "coords_6d" not in known or ("lengths" not in known and "aa_str" not in known):
                raise SystemExit("--inpaint_coords file must hold 'coords_6d' and 'lengths' (or 'aa_str')")
        coords = known["coords_6d"].float()
        if tuple(coords.shape[1:]) != (C_, L_, L_) or coords.shape[0] not in (1, B):
            raise SystemExit(f"coords_6d must be (1 or {B}, {C_}, {L_}, {L_}), got {tuple(coords.shape)}")
        rep = B // coords.shape[0]
        known = {"coords_6d": coords.repeat(rep, 1, 1, 1),
                 **({"lengths": list(known["lengths"]) * rep} if "lengths" in known else {"aa_str": list(known["aa_str"]) * rep})}
        if want_target:
            from text2protein_amd.encode import sse_target
            ss_target = sse_target(known["coords_6d"])

    def to_device(c):
        return {k: to_device(v) if isinstance(v, dict) else v.to(device) for k, v in c.items()}

    for it in range(args.n_iter):
        if args.select_length:
            mask = get_mask_all_lengths(config, batch_size=B)[args.length_index - 1]
            condition = {"length": mask.to(device)}
        elif pdb_condition is not None:
            condition = dict(pdb_condition)
        elif known is not None:
            # sampling_6d.py:146-147 -> get_condition_from_batch (utils.py:84-106): every condition the model was trained with
            condition = to_device(get_condition_from_batch(config, known, mask_info=args.mask_info or "1:5,10:15"))
            if replace:
                condition["_batch"] = {"coords_6d": known["coords_6d"].to(device),
                                       **{k: known[k] for k in ("lengths", "aa_str") if k in known}}
        else:
            condition = {}
        sample, n = sampling_fn(score_model, condition=condition, context=context)
        if dist is not None:
            sample = D.gather_samples(sample, dist)          # the single data-path collective of a run
            all_ids = [None] * world
            dist.all_gather_object(all_ids, ids)
            out_ids = [i for sub in all_ids for i in sub]
        else:
            out_ids = ids
        generated = sample.cpu()
        if rank == 0:
            print("show generated samples shape: ", generated.shape)
            for i, sid in enumerate(out_ids):
                suffix = f"_{it}" if args.n_iter > 1 else ""
                with open(workdir.joinpath(f"sampled_{sid}{suffix}.pkl"), "wb") as f:
                    pkl.dump(generated[i].unsqueeze(0), f)
            if args.decode or args.fold:
                import numpy as np
                from text2protein_amd.decode import NAMES, decode_6d_batch
                lengths, clipped, absval = decode_6d_batch(sample)
                for i, sid in enumerate(out_ids):
                    Lb = int(lengths[i])
                    if Lb < 0:          # sampling_rosetta.py:72-73 raises for such a sample; here it is reported and skipped
                        print(f"sample {sid}: improper masking channel, not decoded")
                        continue
                    suffix = f"_{it}" if args.n_iter > 1 else ""
                    arrs = {}
                    for c, nm in enumerate(NAMES):
                        arrs[nm] = clipped[i, c, :Lb * Lb].reshape(Lb, Lb).cpu().numpy()
                        arrs[nm + "_abs"] = absval[i, c, :Lb * Lb].reshape(Lb, Lb).cpu().numpy()
                    np.savez(workdir.joinpath(f"decoded_{sid}{suffix}.npz"), **arrs)
                if args.fold:
                    import json
                    from text2protein_amd import fold as F
                    xyz, status, placed, diag = F.fold_maps_batch(absval, lengths)
                    xyz_dev, xyz = xyz, xyz.cpu().numpy()
                    fold_dev = xyz_dev
                    chains = F.diagnostics(status, placed, diag, lengths)
                    refined = None
                    if args.refine:                 # minimised against the restraint set; these are the chains scored below
                        from text2protein_amd import refine as R
                        r_rounds = None
                        try:
                            if in_rounds:           # draws: the run's seed, the sample ids, one block of streams per --n_iter call
                                import zlib
                                cids = [int(s) & 0x7FFFFFFF if str(s).isdigit() else zlib.crc32(str(s).encode()) & 0x7FFFFFFF for s in out_ids]
                                xyz_dev, r_status, r_diag, r_trace = R.refine_rounds_batch(
                                    xyz_dev, absval, lengths, args.refine_rounds, args.refine_replicas, seed=args.seed,
                                    stream_base=it * R.STREAM_STRIDE * R.MAX_ROUNDS, chain_ids=cids)
                                r_rounds = R.rounds_diagnostics(r_trace)
                            else:
                                xyz_dev, r_status, r_diag = R.refine_backbone_batch(xyz_dev, absval, lengths)
                        except ValueError as e:
                            raise SystemExit(f"--refine: {e}")
                        refined = xyz_dev.cpu().numpy()
                        for i, (d, r) in enumerate(zip(chains, R.diagnostics(r_status, r_diag, lengths))):
                            d["refine"] = r
                            if r_rounds is not None:
                                d["refine"]["rounds"] = r_rounds[i]
                    if args.ss_check:               # letters of the chains as folded and as refined, against the condition's blocks
                        target = None if ss_target is None else ss_target * world
                        stages = [("folded", F.ss_agreement(fold_dev, lengths, target))]
                        if refined is not None:
                            stages.append(("refined", F.ss_agreement(xyz_dev, lengths, target)))
                        for i, d in enumerate(chains):
                            d["sse"] = {name: rows[i] for name, rows in stages}
                    tm = None
                    if tm_refs is not None:         # every folded chain against every reference, and the samples against each other
                        keep = [i for i, d in enumerate(chains) if d["status"] >= 0]
                        if keep:
                            tm = TM.score_samples(xyz_dev[keep], torch.as_tensor([chains[i]["L"] for i in keep], dtype=torch.int32),
                                                  [out_ids[i] for i in keep], *tm_refs)
                            suffix = f"_{it}" if args.n_iter > 1 else ""
                            with open(workdir.joinpath(f"tm_scores{suffix}.json"), "w") as f:
                                json.dump(tm, f)
                    for i, (sid, d) in enumerate(zip(out_ids, chains)):
                        if d["status"] < 0:         # reported above
                            continue
                        suffix = f"_{it}" if args.n_iter > 1 else ""
                        F.write_backbone_pdb(workdir.joinpath(f"folded_{sid}{suffix}.pdb"), xyz[i, :d["L"]])
                        if refined is not None:
                            F.write_backbone_pdb(workdir.joinpath(f"refined_{sid}{suffix}.pdb"), refined[i, :d["L"]])
                            if d["refine"]["status"] != 0:
                                print(f"sample {sid}: refine status {d['refine']['status']}")
                        with open(workdir.joinpath(f"fold_{sid}{suffix}.json"), "w") as f:
                            json.dump(d, f)
                        if d["status"] != 0:
                            print(f"sample {sid}: fold status {d['status']} ({d['unreachable_pairs']} unreachable pairs, "
                                  f"{len(d['placed'])} residues placed without a frame of their own)")
                        if args.ss_check and ss_target is not None:
                            def pct(v):
                                return "no target" if v is None else f"{100.0 * v:.1f} %"
                            print(f"sample {sid}: secondary structure " + "; ".join(
                                f"{name}: helix {pct(v['helix_agreement'])}, strand {pct(v['strand_agreement'])}" for name, v in d["sse"].items()))
                        if tm is not None:
                            t = tm["samples"][str(sid)]
                            if t["scored"]:
                                print(f"sample {sid}: TM to {len(tm['references'])} references min {t['sample_min']:.4f} max {t['sample_max']:.4f} "
                                      f"avg {t['sample_avg']:.4f} std {t['sample_std']:.4f}, closest {t['closest']} "
                                      f"(TM {t['tm_by_reference']:.4f} by the reference, {t['tm_by_sample']:.4f} by the sample)")
                            else:
                                print(f"sample {sid}: not scored -- " + (f"{t['L']} residues, outside the 5 to 256 TM-align takes"
                                                                          if t["why"] == "sample" else "no reference chain TM-align can take"))
            print(f"[{it + 1} / {args.n_iter}] save samples to {workdir} ({n} score evaluations per chain)")
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
