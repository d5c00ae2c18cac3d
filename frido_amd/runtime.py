"""Runtimes that own compiled HIP programs for a model instance.

  DenoiserRuntime  — PyUNetModel.forward(x, t, context, stage) on the HIP engine (API path);
  SamplerEngine    — the multi-stage DDIM / PLMS loop with per-sample invariants hoisted, the per-step
                     body captured in a hipGraph (one builder, _body, and one replay loop, _replay over replay_units, for every
                     kind), a device step counter and coefficient tables
                     (reference: frido/models/diffusion/ddim.py:116-273, plms.py:116-303); kind="ddpm": the
                     ancestral loop of frido/models/diffusion/frido.py:1308-1418 on the same machinery; kind="dpm":
                     DPM-Solver++(2M), which the reference does not have, in DDIM's loop (frido_dpm_step as the update); kind="invert":
                     DDIM's deterministic encoder, the chain walked upwards from a clean latent (frido_invert_step as the update);
  ancestral_step   — one ancestral update outside a loop (FridoDiffusion.p_mean_variance / p_sample);
  DecoderRuntime   — VQModelInterface.decode / decode_first_stage on the HIP engine; MSFPNVQModel's encode_quant / decode_quant /
                     reconstruct (encode program, codebook loss and decode program as one captured graph).
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, config
from .builder import Builder
from .engine import Prog, current_stream_ptr, own_stream, require_gpu
from .schedules import (ancestral_table, ddim_inversion_table, dpm_solver_table, make_ddim_sampling_parameters, make_ddim_timesteps,
                        sampler_coef_table)
from .unet_plan import UNetStagePlan
from .vqgan_plan import VQDecodePlan, VQDecodeQuantPlan, VQEncodePlan

# step bodies per captured DDIM graph (1 = one graph launch per step, the r01-r05 form; r06 default 20: 10 measured +0.17 %, 40 +0.28 % end to end, interleaved,
# profiles/r06_graph_steps_ab.txt); see SamplerEngine._replay
GRAPH_STEPS = max(1, int(os.environ.get("FRIDO_GRAPH_STEPS", "20")))
GUIDANCE_MAX = 8                          # conditionings per composed engine: the main one and up to 7 of `compose=`
EDIT_RNG_STREAM = 64                      # Philox stream of stage s's blend draws: 64 + s, apart from 0 (x_T) and 1 .. num_stage (the updates)


def _weights_of(module, device):
    return {k: v.detach().to(device=device, dtype=torch.float32).contiguous() for k, v in module.state_dict().items()}


def _run1(builder, kind, stream, **kw):
    """Launch a single op immediately."""
    p = Prog(builder.device, builder.nsplit)
    p.emit(kind, **kw)
    p.run(stream)


def _relayout(builder, st, src, dst, B, HW, Cn, to_nchw, c0=0, Cuse=None, Cdst=None):
    """One NCHW <-> NHWC launch between the tensors src and dst ([B][Cn][HW] <-> [B][HW][Cn]; to_nchw: which way).  c0 / Cuse / Cdst: only
    the channels [c0, c0 + Cuse) of src's Cn, into a dst of Cdst channels (default: all of them, into as many)."""
    Cuse = Cn if Cuse is None else Cuse
    _run1(builder, "FRIDO_OP_RELAYOUT", st, src=src.data_ptr(), dst=dst.data_ptr(), B=B, HW=HW, Csrc=Cn, c0=c0, Cuse=Cuse,
          Cdst=Cuse if Cdst is None else Cdst, d0=0, to_nchw=to_nchw)


def module_builder(module, device, precision):
    """The Builder over `module`'s weights on `device`, for the build of the library `precision` selects (_lib.use_planes)."""
    planes = config.planes(precision)
    with _lib.use_planes(planes):
        device = require_gpu(device)
    return Builder(device, config.nsplit(precision), _weights_of(module, device), planes=planes)


class _Runtime:
    """What a model's runtime starts from: its Builder (`b`) and that builder's device / nsplit / planes, the configuration, no plans."""

    def __init__(self, module, cfg, device, precision=None):
        self.b = module_builder(module, device, precision)
        self.device, self.nsplit, self.planes = self.b.device, self.b.nsplit, self.b.planes
        self.cfg = cfg
        self.plans = {}


class DenoiserRuntime(_Runtime):
    def __init__(self, module, cfg, device, precision=None):
        super().__init__(module, cfg, device, precision)
        self._replicas = {0: self.b}

    def builder_for(self, replica):
        """Builder of sampler replica `replica`.  Replica 0 is the runtime's own; further replicas get their OWN activation
        pool, persistent buffers and split-K workspace (they share the f32 weight tensors, not the scratch), so that their
        captured step bodies can be replayed CONCURRENTLY on different streams (only tools/dual_stream_exp.py does that: the
        measured gain of two concurrent sub-batches was +1 %, so pipeline.sample_images runs ONE replica)."""
        if replica not in self._replicas:
            self._replicas[replica] = Builder(self.device, self.nsplit, self.b.w, ws_tag=f":r{replica}", planes=self.planes)
        return self._replicas[replica]

    @_lib.with_planes
    def forward(self, x, t, context, stage, y=None):
        """x (B, Cin, H, W) f32 cuda NCHW, t (B,) int64, context (B, nctx, cd) or None (AttentionBlock denoisers), y class labels
        ((B,) int64 or (B, num_classes) float) or None -> eps (B, nch, H, W)."""
        B, Cin, H, W = x.shape
        nctx = context.shape[1] if context is not None else 0
        stage = 0 if stage is None else int(stage)
        key = (B, H, W, nctx, stage, Cin)
        st = current_stream_ptr(self.device)
        if key not in self.plans:
            x_state = torch.zeros(B, H * W, Cin, dtype=torch.float32, device=self.device)
            self.plans[key] = UNetStagePlan(self.b, self.cfg, B=B, H=H, W=W, nctx=nctx, stage=stage, x_state=x_state,
                                            temb_rows=B, per_sample_t=True)
        plan = self.plans[key]
        xc = x.contiguous().float()
        _relayout(self.b, st, xc, plan.x_state, B, H * W, Cin, 0)
        if context is not None:
            plan.set_context(context.to(torch.float32))
        if y is not None:
            plan.set_labels(y)
        plan.set_timesteps(t.to(torch.int64))
        plan.pre.run(st)
        plan.step.run(st)
        out = torch.empty(B, plan.nch, H, W, dtype=torch.float32, device=self.device)
        _relayout(self.b, st, plan.eps, out, B, H * W, plan.nch, 1)
        return out


@torch.no_grad()
def ancestral_step(builder, x, eps, rows, coef, start, *, noise=None, temperature=1.0, seed=0, sample0=0, rng_stream=0):
    """One ancestral (DDPM) update on the HIP kernel, outside a sampling loop (frido.py:1246-1258,1286-1305).
    x (B, Cx, H, W) f32 NCHW on the GPU, eps (B, nch, H, W) the denoiser's output for channels [start, start + nch), rows: one row
    index of the device table `coef` ([n][COEF_ROW], schedules.ancestral_table) per sample, noise (B, Cx, H, W) on the GPU or None
    (Philox keyed by (seed, sample0 + b, row + 1, rng_stream)).  Samples that share a row go out in one launch; a non-uniform `t`
    launches per sample.  Returns (x' NCHW, x0 NCHW).  The layout changes around the kernel are FRIDO_OP_RELAYOUT launches."""
    B, Cx, H, W = x.shape
    nch, HW, dev = eps.shape[1], H * W, x.device
    with _lib.use_planes(builder.planes):
        st = current_stream_ptr(dev)

        def nhwc(t):
            t = t.contiguous().float()
            out = torch.empty(B, HW, t.shape[1], dtype=torch.float32, device=dev)
            _relayout(builder, st, t, out, B, HW, t.shape[1], 0)
            return out

        def nchw(t):
            out = torch.empty(B, Cx, H, W, dtype=torch.float32, device=dev)
            _relayout(builder, st, t, out, B, HW, Cx, 1)
            return out
        xs, es = nhwc(x), nhwc(eps)
        ns = nhwc(noise) if noise is not None else None
        xo, p0 = torch.empty_like(xs), torch.empty_like(xs)
        rows = [int(r) for r in rows]
        assert len(rows) == B and all(0 <= r < coef.shape[0] for r in rows)
        spans = [(0, B)] if len(set(rows)) == 1 else [(b, 1) for b in range(B)]
        for b0, nb in spans:
            off = b0 * HW * 4
            kw = dict(x=xs.data_ptr() + off * Cx, B=nb, HW=HW, Cx=Cx, start=start, nch=nch, eps_cond=es.data_ptr() + off * nch,
                      coef=coef.data_ptr(), coef_row_offset=rows[b0], temperature=float(temperature), x_out=xo.data_ptr() + off * Cx,
                      pred_x0=p0.data_ptr() + off * Cx, write_x=1, seed=int(seed), sample0=int(sample0) + b0, rng_stream=int(rng_stream),
                      hist_mode=_lib.STEP_ANCESTRAL)
            if ns is not None:
                kw.update(noise=ns.data_ptr() + off * Cx, noise_stride=0, noise_C=Cx, noise_c0=0)
            _run1(builder, "FRIDO_OP_SAMPLER_STEP", st, **kw)
        return nchw(xo), nchw(p0)


def _unfold_nhwc(builder, st, geo, x, crops=None):
    """x (B, C, H, W) NCHW -> its crops [B * L][kh * kw][C] NHWC, into `crops` if given: FRIDO_OP_RELAYOUT to NHWC, frido_unfold."""
    from .patching import launch_unfold
    B, Cn, H, W = x.shape
    kh, kw = geo.src[2:4]
    xs = torch.empty(B, H * W, Cn, dtype=torch.float32, device=x.device)
    if crops is None:
        crops = torch.empty(B * geo.L, kh * kw, Cn, dtype=torch.float32, device=x.device)
    _relayout(builder, st, x, xs, B, H * W, Cn, 0)
    launch_unfold(geo.unfold_desc(xs.data_ptr(), crops.data_ptr(), B, Cn), st)
    return crops


def _fold_nchw(builder, st, geo, crops, B, Cn):
    """crops [B * L][kh' * kw'][C] NHWC -> their weighted, normalised recombination (B, C, H', W') NCHW: frido_fold, FRIDO_OP_RELAYOUT."""
    from .patching import launch_fold
    H, W = geo.out[:2]
    fs = torch.empty(B, H * W, Cn, dtype=torch.float32, device=crops.device)
    out = torch.empty(B, Cn, H, W, dtype=torch.float32, device=crops.device)
    launch_fold(geo.fold_desc(crops.data_ptr(), fs.data_ptr(), B, Cn), st)
    _relayout(builder, st, fs, out, B, H * W, Cn, 1)
    return out


@torch.no_grad()
def patch_unfold(builder, geo, x, out=None):
    """x (B, C, H, W) f32 NCHW on the GPU -> its crops (B * L, C, kh, kw) NCHW, into `out` if given (patching.PatchGeometry `geo`; crop l
    of sample b at b * L + l): FRIDO_OP_RELAYOUT to NHWC, frido_unfold, FRIDO_OP_RELAYOUT back."""
    B, Cn, H, W = x.shape
    _, _, kh, kw, _, _ = geo.src
    assert (H, W) == geo.src[:2]
    Bc = B * geo.L
    with _lib.use_planes(builder.planes):
        st = current_stream_ptr(x.device)
        cs = _unfold_nhwc(builder, st, geo, x.contiguous())
        if out is None:
            out = torch.empty(Bc, Cn, kh, kw, dtype=torch.float32, device=x.device)
        _relayout(builder, st, cs, out, Bc, kh * kw, Cn, 1)
    return out


@torch.no_grad()
def patch_fold(builder, geo, o, B):
    """o (B * L, C, kh', kw') f32 NCHW crops -> the weighted, normalised recombination (B, C, H', W') NCHW (the fold side of `geo`)."""
    Bc, Cn = o.shape[:2]
    _, _, kh, kw, _, _ = geo.out
    assert Bc == B * geo.L and tuple(o.shape[2:]) == (kh, kw), (tuple(o.shape), B, geo.L, kh, kw)
    with _lib.use_planes(builder.planes):
        st = current_stream_ptr(o.device)
        cs = torch.empty(Bc, kh * kw, Cn, dtype=torch.float32, device=o.device)
        _relayout(builder, st, o.contiguous().float(), cs, Bc, kh * kw, Cn, 0)
        return _fold_nchw(builder, st, geo, cs, B, Cn)


def logged_at(n, log_every_t):
    """i -> whether the result of step i of n is logged, which needs the host: the reference's `index % log_every_t == 0 or index == n - 1`
    with index = n - 1 - i (ddim.py:177, plms.py:190; frido.py:1409 with index = t)."""
    return lambda i: (n - 1 - i) % log_every_t == 0 or i == 0


def replay_units(n, K, host_at, i0=0):
    """The lengths of the units the steps i0 ... n - 1 of n are replayed in.  A K-step graph exists where K > 1 and n - i0 >= K; step i
    starts a K-unit where one exists, i + K <= n and none of the steps i ... i + K - 2 needs the host (host_at(j): its result is logged) -- a
    step that does may only END a unit.  Every other unit is one step."""
    units, i = [], i0
    while i < n:
        fits = K > 1 and n - i0 >= K and i + K <= n and not any(host_at(j) for j in range(i, i + K - 1))
        units.append(K if fits else 1)
        i += units[-1]
    return units


def stage_masks(mask, num_stage):
    """A keep mask (B, 1, H, W) in [0, 1] (1 = keep) -> one mask per stage: stage s works on a grid 2^(num_stage - 1 - s) times coarser
    (its result is block-averaged by the hand-off), so it uses the mask's MIN over those blocks, expanded back by nearest -- a coarse cell
    is kept only if all of it is kept, and the hand-off's block mean never mixes kept and regenerated values.  Torch on the tiny mask,
    once per call."""
    out = []
    for s in range(num_stage):
        f = 2 ** (num_stage - 1 - s)
        if f == 1:
            out.append(mask)
            continue
        if mask.shape[2] % f or mask.shape[3] % f:
            raise ValueError(f"a {mask.shape[2]} x {mask.shape[3]} mask does not split into the {f} x {f} blocks of stage {s}")
        m = -torch.nn.functional.max_pool2d(-mask, f, f)
        out.append(torch.nn.functional.interpolate(m, scale_factor=f, mode="nearest"))
    return out


class EditSpec:
    """What SamplerEngine.run(edit=) needs to edit a latent instead of sampling one.
    z0 (B, C, H, W): the clean latent, on the device.  k: steps per stage, the LAST k rows of the S-row chain.  sqrt_ac / sqrt_1mac: the
    model's own sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod buffers (q_sample's coefficients).  masks: None or one (B, 1, H, W)
    device mask per stage (stage_masks).  init: "z0" -- every stage starts from q_sample of z0's stage channels at the chain's first
    timestep -- or "noise" (x_T or a draw).  blend: the window of every blend, "stage" = the stage's own channels [a_s, e_s), "reference"
    = [0, e_s).  reimpose: a last noise-free blend after the stage's steps.  first_stage: stages below it keep the start state's channels."""

    def __init__(self, z0, k, sqrt_ac, sqrt_1mac, masks=None, init="z0", blend="stage", reimpose=True, first_stage=0):
        assert init in ("z0", "noise") and blend in ("stage", "reference"), (init, blend)
        self.z0, self.k, self.sqrt_ac, self.sqrt_1mac, self.masks = z0, int(k), sqrt_ac, sqrt_1mac, masks
        self.init, self.blend, self.reimpose, self.first_stage = init, blend, bool(reimpose), int(first_stage)


class SamplerEngine:
    """One instance per (denoiser weights, B, latent shape, context length, S, eta, cfg on/off, kind, patch geometry).

    Every kind runs the same way: _bind_stage, then a step body ([model evaluation, _update_op, counter add], built and captured once per
    (form, stage) by _body and kept in `graphs`) replayed by _replay in the units of replay_units.  A score corrector, an arbitrary Python
    hook between the denoiser and the update, makes a stage run eagerly instead: forward program, _corrected_eps, update program.

    patch (a split_input_params dict; DDIM / PLMS only): the patch-wise mode of frido.py:1076-1152.  The state x, pred_x0, the PLMS eps
    ring, the stage hand-off and the update kernel stay on the FULL latent; the stage plans are built for the B * L crops (kh x kw) and
    read a crop buffer, and every model evaluation is frido_unfold(x -> crops) -> step program -> frido_fold(crop eps -> full eps), all
    inside the captured step body.  A stage's `pre` program reads the crop buffer too (the SPADE maps come from the
    frozen channels), so an unfold precedes it.  Memory: everything per-sample in the plans -- activations, the SPADE maps and the
    cross-attention K / V^T caches (B * L * xrep rows) -- is L times the whole-latent engine's at the crop size.

    ncond / rescale: an engine is COMPOSED when ncond > 1 or rescale.  Its plans evaluate xrep = ncond + 1 conditionings per step --
    [c_0 | ... | c_{ncond-1} | uncond] -- and every model evaluation is followed by frido_guidance_compose, which mixes them in place into
    slot 0 with the device weights guide_w (w_0 .. w_{ncond-1}, then the rescale factor phi: run(weights=, phi=) fills them, so other values
    replay the same graphs); the update kernel then reads slot 0 as an already mixed eps (the score corrector's route), whatever its kind.
    Memory: everything per-sample in the plans -- activations, SPADE maps, K / V^T caches, a class-conditional denoiser's S * Bx embedding
    table -- is (ncond + 1) / 2 times the classifier-free engine's.  A non-composed engine has none of this: same ops, buffers and graphs."""

    def __init__(self, builder: Builder, cfg, **kw):
        self.planes = builder.planes
        with _lib.use_planes(self.planes):
            self._init(builder, cfg, **kw)

    def _init(self, builder: Builder, cfg, *, B, C, H, W, nctx, S, eta, kind, alphas_cumprod, embed_dim, cfg_scale=1.0,
              use_graph=True, num_stage=None, temperature=1.0, posterior=None, clip=False, patch=None, order=2, skip_type="logSNR",
              lower_order_final=True, ncond=1, rescale=False, compose_always=False):
        self.b, self.cfg = builder, cfg
        self.dev = builder.device
        self.B, self.C, self.H, self.W, self.nctx = B, C, H, W, nctx
        self.kind = kind
        self.cfg_scale = float(cfg_scale)
        self.xrep = 2 if self.cfg_scale != 1.0 else 1
        self.ncond, self.rescale = int(ncond), bool(rescale)
        # compose_always: one conditioning without rescale through the composed route all the same (tools/compose_step_bench.py measures
        # the route's own cost with it; no public call sets it)
        self.composed = self.ncond > 1 or self.rescale or bool(compose_always)
        if self.composed:
            assert 1 <= self.ncond <= GUIDANCE_MAX, f"1 to {GUIDANCE_MAX} conditionings, got {ncond}"
            assert kind in ("ddim", "plms", "dpm") and patch is None, "composed guidance is built for the whole-latent DDIM / PLMS / DPM-Solver loops"
            self.xrep = self.ncond + 1
            self.guide_w = torch.zeros(self.ncond + 1, dtype=torch.float32, device=builder.device)      # the weights, then phi
        self.embed = list(embed_dim)
        self.num_stage = num_stage if num_stage is not None else cfg.get("num_stage", 1)
        self.use_graph = use_graph
        self.temperature = float(temperature)
        if kind == "ddpm":
            # frido.py:1391-1394: every stage walks t = S - 1 ... 0 (S = num_timesteps, `timesteps=` or `start_T`); `posterior`: ddpm_tables' arrays
            # The device table holds the WHOLE schedule (row r: t = num_timesteps - 1 - r) and a chain of S steps starts at row row0: the
            # kernel's Philox draw index is its row + 1 = num_timesteps - t, whatever S is -- the key FridoDiffusion.p_sample uses too
            tab, self.t_loop = ancestral_table(posterior, None, clip_denoised=clip), np.arange(S - 1, -1, -1)
            assert 0 < S <= tab.shape[0], f"ancestral chain of {S} steps on a schedule of {tab.shape[0]}"
            self.row0 = tab.shape[0] - S
        elif kind == "dpm":
            # DPM-Solver++(2M): the grid (skip_type) is part of the solver; every stage walks the table from row 0, a first-order row
            assert patch is None, "the DPM-Solver loop has no patch-wise mode"
            self.t_loop, tab = dpm_solver_table(np.asarray(alphas_cumprod, dtype=np.float64), S, skip_type, order, lower_order_final)
        elif kind == "invert":
            # DDIM's chain walked UPWARDS: row i = the sampler's ddim_alphas / ddim_alphas_prev / ddim_timesteps at index i, so the
            # time-embedding rows and the coefficient rows ascend together and the device counter still only increments
            assert patch is None, "the inversion loop has no patch-wise mode"
            ac32 = np.asarray(alphas_cumprod, dtype=np.float32)
            self.t_loop = make_ddim_timesteps("uniform", S, len(ac32))
            _, al, alp = make_ddim_sampling_parameters(ac32, self.t_loop, 0.0)
            tab = ddim_inversion_table(al, alp)
        else:
            tab, self.t_loop = sampler_coef_table(np.asarray(alphas_cumprod, dtype=np.float32), S, eta, plms=(kind == "plms"))
        self.n_steps = S if kind == "ddpm" else tab.shape[0]
        self.coef = torch.from_numpy(tab).to(self.dev)
        self.step = torch.zeros(1, dtype=torch.int32, device=self.dev)
        # class-conditional denoisers: the embedding table has one row per (step, sample); this counter advances by Bx per step
        self.labels = cfg.get("num_classes") is not None
        self.step_bx = torch.zeros(1, dtype=torch.int32, device=self.dev) if self.labels else None
        self.rng = torch.zeros(2, dtype=torch.int64, device=self.dev)   # {seed, sample0} read by the captured kernels
        self.cfg_dev = torch.ones(1, dtype=torch.float32, device=self.dev)   # guidance scale read by the captured kernels
        if not cfg.get("use_split_head", False):
            raise NotImplementedError("SamplerEngine: the multi-stage loop masks channels per stage, which needs "
                                      "use_split_head=True (every shipped Frido config)")
        self.x = torch.zeros(B, H * W, C, dtype=torch.float32, device=self.dev)
        self.pred_x0 = torch.zeros_like(self.x)
        self.geo = None
        self.Bm, (Hm, Wm), x_model = B, (H, W), self.x      # what the stage plans see: the latent, or (patch mode) its B * L crops
        if patch is not None:
            from . import patching
            assert kind != "ddpm", "the ancestral loop has no patch-wise mode"
            self.geo = patching.geometry(patch, H, W, patching.MODEL, self.dev)
            self.Bm, (Hm, Wm) = B * self.geo.L, self.geo.src[2:4]
            self.x_crops = x_model = torch.zeros(self.Bm, Hm * Wm, C, dtype=torch.float32, device=self.dev)
            self.unfold_x = self.geo.unfold_desc(self.x.data_ptr(), self.x_crops.data_ptr(), B, C)
            self.eps_full = []      # per stage: the folded eps [xrep][B][H * W][nch] the update kernel reads
        self.stages = []
        with self.b.persist_scope() as owned:       # this engine owns its plans' persistent buffers: evicting it frees them
            for s in range(self.num_stage):
                plan = UNetStagePlan(self.b, cfg, B=self.Bm, H=Hm, W=Wm, nctx=nctx, stage=s, x_state=x_model, temb_rows=self.n_steps,
                                     per_sample_t=False, step_ptr=self.step.data_ptr(), xrep=self.xrep,
                                     step_bx_ptr=self.step_bx.data_ptr() if self.labels else None)
                self.stages.append(plan)
                if self.geo is not None:
                    self.eps_full.append(torch.zeros(self.xrep * B * H * W, plan.nch, dtype=torch.float32, device=self.dev))
        self._persist = owned
        self.graphs = {}                # step bodies by (form, stage[, "x<K>"]): captured graphs, or (use_graph=False) the programs themselves
        self.graph_captures = 0         # bodies built
        self.multi_step_launches = 0    # K-step units replayed (tests: the K-step graph really ran)
        self._last_logged_stage = None
        self._tape_bufs = {}            # DDIM host noise: the stage's whole tape [n][B][H][W][Cs], at a fixed address
        self._stream = None
        # PLMS state
        if kind == "plms":
            nmax = max(self.embed[:self.num_stage])
            self.hist_stride = B * H * W * nmax
            self.hist = torch.zeros(4, self.hist_stride, dtype=torch.float32, device=self.dev)    # eps ring, slot = step & 3
            self.x_save = torch.zeros_like(self.x)
        if kind == "dpm":
            # the previous step's x0 prediction, one buffer per stage [B * HW][nch]; zero until the stage's first step has run
            self.x0_hist = [torch.zeros(B * H * W, self.embed[s], dtype=torch.float32, device=self.dev) for s in range(self.num_stage)]
        if kind == "ddpm":
            # host-noise form: the tape and the coefficient rows of ONE replay unit (up to GRAPH_STEPS steps), read through a counter of
            # their own that restarts with every unit -- a T = 1000 tape of a whole stage would be gigabytes at B = 16
            self.unit = GRAPH_STEPS if use_graph else 1
            self.step_c = torch.zeros(1, dtype=torch.int32, device=self.dev)
            self.coef_c = torch.zeros(self.unit, tab.shape[1], dtype=torch.float32, device=self.dev)
            self.tape = None

    # ---- the parts of a step body ------------------------------------------------------------------
    def _step_add(self, prog, delta):
        """Advance the device step counter (and, for a class-conditional denoiser, the per-sample table counter by delta * Bx)."""
        prog.emit("FRIDO_OP_STEP_ADD", step=self.step.data_ptr(), delta=delta)
        if self.labels:
            prog.emit("FRIDO_OP_STEP_ADD", step=self.step_bx.data_ptr(), delta=delta * self.Bm * self.xrep)

    def _prog(self, ops=()):
        """A program for a step body, filled from `ops`: a (kind name, fields) pair is one op, a list holds finished ops (a model
        evaluation: _eval_ops), an int advances the step counter."""
        p = Prog(self.dev, self.b.nsplit)
        for op in ops:
            if isinstance(op, int):
                self._step_add(p, op)
            elif isinstance(op, list):
                p.ops += op
            else:
                p.emit(op[0], **op[1])
        return p

    def _eval_ops(self, s):
        """The ops of ONE model evaluation at stage s, leaving eps where _eps_ptr(s) points -- on a composed engine the guidance-mixed
        eps, in slot 0 of the xrep evaluations."""
        plan = self.stages[s]
        if self.composed:
            eps = self._eps_ptr(s)
            mix = _lib.make_op("FRIDO_OP_GUIDANCE_COMPOSE", eps=eps, out=eps, weights=self.guide_w.data_ptr(), n=self.ncond, B=self.B,
                               per_sample=self.H * self.W * plan.nch, rescale=int(self.rescale))
            return list(plan.step.ops) + [mix]
        if self.geo is None:
            return list(plan.step.ops)
        fold = self.geo.fold_desc(plan.eps.data_ptr(), self.eps_full[s].data_ptr(), self.xrep * self.B, plan.nch)
        return [_lib.op_of("FRIDO_OP_UNFOLD", self.unfold_x)] + list(plan.step.ops) + [_lib.op_of("FRIDO_OP_FOLD", fold)]

    def _eps_ptr(self, s):
        return (self.eps_full[s] if self.geo is not None else self.stages[s].eps).data_ptr()

    def _update_op(self, s, noise=None, hist_mode=0, no_cfg=False):
        """(kind name, fields) of stage s's state update on the engine's buffers, for its kind: the DDIM / PLMS step (hist_mode: how PLMS uses
        its eps ring), the ancestral step, the DPM-Solver++ step with the stage's x0 history, or the inversion step.  noise: None -- Philox in
        the kernel, keyed by the device {seed, sample0} -- or (address, channels) of host noise [step][B][HW][channels] read by step index.
        no_cfg: the eps is already guidance-mixed (a score corrector ran); a composed engine's always is."""
        B, HW, C = self.B, self.H * self.W, self.C
        start, nch, eps = sum(self.embed[:s]), self.embed[s], self._eps_ptr(s)
        cfg2 = not self.composed and self.xrep == 2      # the update kernel mixes [cond | uncond] itself
        if self.kind == "invert":       # the stage's window only, no noise, no x0
            return "FRIDO_OP_INVERT_STEP", dict(
                x=self.x.data_ptr(), eps_cond=eps, eps_uncond=eps + 4 * B * HW * nch if cfg2 else None, cfg_scale=self.cfg_scale,
                cfg_dev=self.cfg_dev.data_ptr(), coef=self.coef.data_ptr(), step=self.step.data_ptr(), B=B, HW=HW, Cx=C, c_lo=start,
                c_hi=start + nch)
        kw = dict(x=self.x.data_ptr(), B=B, HW=HW, Cx=C, start=start, nch=nch, eps_cond=eps, coef=self.coef.data_ptr(),
                  step=self.step.data_ptr(), x_out=self.x.data_ptr(), pred_x0=self.pred_x0.data_ptr())
        if self.kind != "ddpm":
            kw.update(cfg_scale=self.cfg_scale, cfg_dev=self.cfg_dev.data_ptr())
            if cfg2 and not no_cfg:
                kw["eps_uncond"] = eps + 4 * B * HW * nch
        if self.kind == "dpm":
            return "FRIDO_OP_DPM_STEP", dict(kw, x0_hist=self.x0_hist[s].data_ptr())
        kw.update(write_x=1, temperature=self.temperature, rng_stream=s + 1, rng_dev=self.rng.data_ptr())
        if noise is not None:
            kw.update(noise=noise[0], noise_stride=B * HW * noise[1], noise_C=noise[1], noise_c0=start)
        if self.kind == "ddpm":
            kw["hist_mode"] = _lib.STEP_ANCESTRAL
            if noise is None:
                kw["coef_row_offset"] = self.row0
            else:     # this unit's noise (already multiplied by its temperature) and coefficient rows, by the unit's own counter
                del kw["rng_stream"], kw["rng_dev"]
                kw.update(coef=self.coef_c.data_ptr(), step=self.step_c.data_ptr(), temperature=1.0, noise_c0=0)
        elif hist_mode:
            kw.update(hist_ring=self.hist.data_ptr(), hist_stride=self.hist_stride, hist_mode=hist_mode)
        return "FRIDO_OP_SAMPLER_STEP", kw

    def _body(self, key, sp, build_ops):
        """The step body kept under `key` = (form, stage[, "x<K>"]), built on first use from build_ops(): captured, or (use_graph=False) the
        program itself."""
        if key not in self.graphs:
            p = self._prog(build_ops())
            p.keep = [self.stages[key[1]]]
            self.graphs[key] = p.capture(sp) if self.use_graph else p
            self.graph_captures += 1
        return self.graphs[key]

    def _go(self, g, sp):
        g.launch(sp) if self.use_graph else g.run(sp)

    def _replay(self, key, K, host_at, sp, before_unit=None, after_unit=None, first=None, n=None, i0=0):
        """All n steps of a stage from the body under `key`, in the units of replay_units.  K > 1: the same body K times in ONE captured graph
        (the device step counter makes every repetition pick its own timestep / noise slice), replayed wherever the K - 1 steps in between need
        no host access: fewer graph launches -- the trace shows ~30 us between the last kernel of one replay and the first of the next
        (profiles/r05_x3_gap_analysis.json).  before_unit(i, length) / after_unit(last step) are the kind's host work around a unit; `first`:
        the body of step 0 where it differs (PLMS).  n / i0 (an edit): the steps i0 ... n - 1 of a chain of n <= n_steps; the device counter
        is where the chain left it, so the same bodies serve every start row."""
        n, g = self.n_steps if n is None else n, self.graphs[key]
        # (Graph.keep = (packed descriptor array, the program it was captured from))
        gk = self._body(key + ("x%d" % K,), sp, lambda: [list(g.keep[1].ops) * K]) if K > 1 and n - i0 >= K else None
        i = i0
        for unit in replay_units(n, K, host_at, i0):
            if before_unit is not None:
                before_unit(i, unit)
            if unit > 1:
                self._go(gk, sp)
                self.multi_step_launches += 1
            else:
                self._go(first if first is not None and i == 0 else g, sp)
            i += unit
            after_unit(i - 1)

    # ---- what a run and a stage start with ----------------------------------------------------------
    @staticmethod
    def _host_draw(noise):
        """shape -> tensor for the host-noise forms ("torch": torch's global CPU generator; a callable: a recorded tape), None for "philox"."""
        return (lambda shape: torch.randn(shape)) if noise == "torch" else (noise if callable(noise) else None)

    def _context(self, cond, uncond=None):
        """cond on the device: the cross-attention context (SpatialTransformer denoisers), class labels (class-conditional ones) or None;
        under classifier-free guidance [cond | uncond]; on a composed engine cond is the sequence (c_0, ..., c_{ncond-1}) and the result
        [c_0 | ... | c_{ncond-1} | uncond]."""
        if self.composed:
            assert len(cond) == self.ncond and uncond is not None, "a composed engine takes its ncond conditionings and the unconditional one"
            first = cond[0]
            dt = torch.float32 if not self.labels or first.is_floating_point() else torch.int64
            return torch.cat([c.to(self.dev, dt) for c in cond] + [uncond.to(self.dev, dt)], dim=0)
        ctx = cond.to(self.dev, torch.float32 if not self.labels or cond.is_floating_point() else torch.int64) if cond is not None else None
        if self.xrep == 2:
            assert ctx is not None, "classifier-free guidance needs a conditioning"
            ctx = torch.cat([ctx, uncond.to(self.dev, ctx.dtype)], dim=0)
        return ctx

    def _init_x(self, x_T, draw, seed, sample0, sp):
        """The start of the chain (ddim.py:127-130): the given x_T, a host draw, or Philox on the device."""
        B, C, H, W = self.B, self.C, self.H, self.W
        xt = x_T if x_T is not None else draw((B, C, H, W)) if draw is not None else None
        if xt is not None:
            xd = torch.as_tensor(xt, dtype=torch.float32).to(self.dev).contiguous()
            assert xd.shape == (B, C, H, W), (tuple(xd.shape), (B, C, H, W))
            _relayout(self.b, sp, xd, self.x, B, H * W, C, 0)
        else:
            _run1(self.b, "FRIDO_OP_RANDN", sp, dst=self.x.data_ptr(), n=B * H * W * C, per_sample=H * W * C, seed=seed, sample0=sample0,
                  rng_stream=0)

    def _per_crop(self, t):
        """A per-sample input of the model ([xrep * B, ...]) repeated for its L crops (crop l of sample b is entry b * L + l)."""
        return t.repeat_interleave(self.geo.L, dim=0) if self.geo is not None and t is not None else t

    def _bind_stage(self, s, ctx, t_loop, sp, row0=0):
        """Stage s's plan on this run's conditioning and timesteps, the step counters at row0 (0: the whole chain; an edit of k steps starts
        at row n_steps - k, and the time-embedding rows follow the same counter), the per-sample invariants (`pre`) computed."""
        plan = self.stages[s]
        if self.labels:
            plan.set_labels(self._per_crop(ctx))
        elif ctx is not None:
            plan.set_context(self._per_crop(ctx))
        plan.set_timesteps(t_loop)
        self.step.fill_(row0)
        if self.labels:
            self.step_bx.fill_(row0 * self.Bm * self.xrep)
        if self.geo is not None:
            from .patching import launch_unfold
            launch_unfold(self.unfold_x, sp)
        plan.pre.run(sp)

    def _to_nchw(self, nhwc, sp):
        out = torch.empty(self.B, nhwc.shape[-1], self.H, self.W, dtype=torch.float32, device=self.dev)
        _relayout(self.b, sp, nhwc, out, self.B, self.H * self.W, nhwc.shape[-1], 1)
        return out

    def _upload_noise(self, s, tape, row0=0, key=None):
        """tape: list of per-step NCHW tensors (B, 3(s+1), H, W) in draw order -> (address, channels) of the stage's persistent NHWC device
        buffer of n_steps rows (fixed address: the captured step body of the tape mode reads it by step index).  row0: the row of the
        tape's first entry (an edit's chain starts there); key: a buffer of its own beside the update's (the blend draws of an edit)."""
        Cs = sum(self.embed[:s + 1])
        key = s if key is None else key
        t = torch.stack([torch.as_tensor(n, dtype=torch.float32) for n in tape])     # [n][B][Cs][H][W]
        assert t.shape[1:] == (self.B, Cs, self.H, self.W) and row0 + t.shape[0] <= self.n_steps, (t.shape, Cs, row0)
        if key not in self._tape_bufs:
            self._tape_bufs[key] = torch.zeros(self.n_steps, self.B, self.H, self.W, Cs, dtype=torch.float32, device=self.dev)
        self._tape_bufs[key][row0:row0 + t.shape[0]].copy_(t.permute(0, 1, 3, 4, 2), non_blocking=False)      # plumbing: layout + H2D
        return self._tape_bufs[key].data_ptr(), Cs

    def _corrected_eps(self, s, sp, t_value, o):
        """`score_corrector.modify_score(model, e_t, x, t, c, **kwargs)` (ddim.py:228-230, plms.py:236-238, frido.py:1233-1241) on the eps the
        forward program just wrote: CFG mix (ddim.py:226), zero-padded like the reference's e_t -- to the channels reached so far, in the
        ancestral loop to the latent's -- hook on torch tensors (NCHW), the stage's channels written back as the (already mixed) conditional
        eps the update kernel reads."""
        plan = self.stages[s]
        B, H, W = self.B, self.H, self.W
        start, nch = sum(self.embed[:s]), self.embed[s]
        Cp = self.C if self.kind == "ddpm" else start + nch
        e = plan.eps.view(self.xrep, B, H, W, nch).permute(0, 1, 4, 2, 3)            # [cond | uncond] x (B, nch, H, W)
        e_t = e[0] if self.xrep == 1 else e[1] + self.cfg_scale * (e[0] - e[1])
        e_t = torch.cat((torch.zeros(B, start, H, W, device=self.dev), e_t, torch.zeros(B, Cp - start - nch, H, W, device=self.dev)), dim=1)
        x_now = self._to_nchw(self.x, sp)[:, :Cp]
        t = torch.full((B,), int(t_value), device=self.dev, dtype=torch.long)
        e_new = o.score_corrector.modify_score(o.model, e_t, x_now, t, o.cond, **o.corrector_kwargs)
        e_new = e_new.to(torch.float32).contiguous()
        assert e_new.shape == (B, Cp, H, W), "modify_score must return a tensor of e_t's shape"
        _relayout(self.b, sp, e_new, plan.eps, B, H * W, Cp, 0, c0=start, Cuse=nch, Cdst=nch)

    # ---- DDIM / PLMS / DPM-Solver++ ----------------------------------------------------------------
    @torch.no_grad()
    @_lib.with_planes
    def run(self, cond, uncond=None, *, x_T=None, noise="philox", seed=0, sample0=0, log_every_t=100, callback=None,
            img_callback=None, noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, model=None, edit=None, weights=None,
            phi=0.0):
        """Runs all stages.  noise: "philox" (device counter RNG), "torch" (draw from torch's global CPU generator in
        exactly the reference's order -- the stream of a reference run on CPU with the same torch.manual_seed), or a
        callable shape -> tensor replaying a recorded tape.  A supplied x_T is, like in the reference (ddim.py:150-152,
        plms.py:150-152), taken as the FINISHED stage-0 result: stage 0 and its pooling hand-off are skipped (with one
        stage x_T comes back unchanged).
        noise_dropout (ddim.py:260-262; plms.py get_x_prev_and_pred_x0): F.dropout of the update's noise -- its keep mask comes from
        torch's generator right after the randn, so it exists in the host-noise modes only ("torch" / a tape).
        score_corrector (ddim.py:228-230): an arbitrary Python hook between the denoiser and the update -- a stage then runs
        step by step on the stream (forward program, hook on torch tensors, update kernel) instead of replaying a captured graph.
        edit (an EditSpec; kind "ddim", whole-latent engines): img2img / keep-mask inpainting, see _edit_stage.  Every stage from
        edit.first_stage on runs the LAST edit.k steps of the chain; the stages below it keep the start state's channels (no steps, no
        hand-off: what an adopted x_T gets), and x_T is only the start state of init="noise", it adopts nothing by itself.
        weights / phi (a composed engine; cond is then the sequence of its ncond conditionings): this run's ncond guidance weights and its
        rescale factor, written to the device vector the captured frido_guidance_compose launches read.
        Returns (samples NCHW, intermediates dict)."""
        assert self.kind != "ddpm", "an ancestral engine runs through run_ancestral()"
        assert self.composed == (weights is not None), "weights= belongs to a composed engine, and a composed engine needs it"
        if self.composed:
            assert len(weights) == self.ncond and score_corrector is None, "ncond weights; a composed engine has no score_corrector hook"
            assert self.rescale or phi == 0.0, "phi needs an engine built with rescale=True"
        assert self.kind != "invert", "an inversion engine runs through run_invert()"
        if edit is not None:
            assert self.kind == "ddim" and self.geo is None, "editing is built for the whole-latent DDIM engine"
            assert noise_dropout == 0. and score_corrector is None, "an edit has no noise_dropout / score_corrector"
            assert 1 <= edit.k <= self.n_steps and 0 <= edit.first_stage < self.num_stage, (edit.k, edit.first_stage)
        if self.kind == "dpm" and (noise_dropout > 0. or score_corrector is not None):
            raise NotImplementedError("the DPM-Solver loop is deterministic and has no hook between the denoiser and the update: "
                                      "noise_dropout / score_corrector are not built for it")
        if noise_dropout > 0. and noise == "philox":
            raise NotImplementedError("noise_dropout draws its keep mask from torch's generator: use noise='torch' (or a recorded tape)")
        if score_corrector is not None and self.geo is not None:
            from .patching import refuse
            raise refuse("score_corrector")
        o = SimpleNamespace(draw=self._host_draw(noise), seed=seed, sample0=sample0, log_every_t=log_every_t, callback=callback,
                            img_callback=img_callback, noise_dropout=float(noise_dropout), score_corrector=score_corrector,
                            corrector_kwargs=dict(corrector_kwargs or {}), model=model, cond=cond, temps=None, edit=edit,
                            n=edit.k if edit is not None else self.n_steps)
        o.row0 = self.n_steps - o.n
        with own_stream(self, self.dev) as sp:
            ctx = self._context(cond, uncond)
            self.cfg_dev.fill_(self.cfg_scale)
            if self.composed:
                self.guide_w.copy_(torch.tensor([float(w) for w in weights] + [float(phi)], dtype=torch.float32))
            if edit is not None:
                self._bind_edit(edit, sp)
            if edit is not None and edit.init == "z0":
                self.x.copy_(self.z0)           # every stage noises its own window of this; the stages below first_stage keep it
            else:
                self._init_x(x_T, o.draw, seed, sample0, sp)
            x0_nchw = self._to_nchw(self.x, sp)
            o.inter = {"x_inter": [x0_nchw], "pred_x0": [x0_nchw]}
            t_loop = torch.from_numpy(self.t_loop.astype(np.int64)).to(self.dev)
            for s in range(self.num_stage):
                if (x_T is not None and s == 0) if edit is None else s < edit.first_stage:
                    continue                 # ddim.py:150-152: "Auto adopt x_T into stage 0" (no denoising, no hand-off)
                self._bind_stage(s, ctx, t_loop, sp, o.row0)
                (self._plms_stage if self.kind == "plms" else self._edit_stage if edit is not None else self._ddim_stage)(s, sp, o)
                levels = self.num_stage - s - 1
                if levels > 0:
                    c0, c1 = sum(self.embed[:s]), sum(self.embed[:s + 1])
                    _run1(self.b, "FRIDO_OP_HANDOFF", sp, x=self.x.data_ptr(), B=self.B, H=self.H, W=self.W, Cx=self.C, c0=c0, c1=c1,
                          levels=levels)
                    # the reference mutates the logged tensor in place (ddim.py:185): mirror that
                    if o.inter["x_inter"] and self._last_logged_stage == s:
                        o.inter["x_inter"][-1] = self._to_nchw(self.x, sp)[:, :c1]
            out = self._to_nchw(self.x, sp)
        return out, o.inter

    def _log(self, s, i, sp, o):
        n, Cs = o.n, sum(self.embed[:s + 1])
        if o.callback:
            o.callback(i)
        if o.img_callback:
            o.img_callback(self._to_nchw(self.pred_x0, sp)[:, :Cs], i)
        if logged_at(n, o.log_every_t)(i):
            o.inter["x_inter"].append(self._to_nchw(self.x, sp)[:, :Cs])
            o.inter["pred_x0"].append(self._to_nchw(self.pred_x0, sp)[:, :Cs])
            self._last_logged_stage = s if i == n - 1 else None

    def _unit_steps(self, o, K):
        """Steps per replay unit: callbacks want the host after every step, and only captured bodies are chained."""
        return K if self.use_graph and o.callback is None and o.img_callback is None else 1

    def _ddim_stage(self, s, sp, o):
        """ddim.py:155-175.  ONE step body per stage (denoiser forward + state update + step-counter bump) is replayed every step: the
        Philox form draws its noise in the update kernel, the tape form (recorded / torch-CPU noise) reads the stage's persistent noise
        buffer by step index.  DPM-Solver++(2M): no noise after x_T (the host generator is left alone), frido_dpm_step as the update."""
        plan, n, noise = self.stages[s], self.n_steps, None
        if self.kind == "ddim" and o.draw is not None:
            # dropout(sigma * noise * temperature) = sigma * temperature * dropout(noise): applied to the host tape, mask drawn right after
            # the step's randn like the reference does
            drop = (lambda z: torch.nn.functional.dropout(z, p=o.noise_dropout)) if o.noise_dropout > 0. else (lambda z: z)
            noise = self._upload_noise(s, [drop(o.draw((self.B, sum(self.embed[:s + 1]), self.H, self.W))) for _ in range(n)])
        elif self.kind == "ddim":
            self.rng.copy_(torch.tensor([o.seed, o.sample0], dtype=torch.int64))
        log = lambda i: self._log(s, i, sp, o)
        if o.score_corrector is not None:       # ddim.py:188-273 with the hook between the (CFG-mixed) eps and the update
            upd = self._prog([self._update_op(s, noise, no_cfg=True), 1])
            for i in range(n):
                plan.step.run(sp)
                self._corrected_eps(s, sp, self.t_loop[i], o)
                upd.run(sp)
                log(i)
            return
        key = ("dpm" if self.kind == "dpm" else "ddim_tape" if noise else "ddim", s)
        self._body(key, sp, lambda: [self._eval_ops(s), self._update_op(s, noise), 1])
        self._replay(key, self._unit_steps(o, GRAPH_STEPS), logged_at(n, o.log_every_t), sp, after_unit=log)

    # ---- DDIM inversion: the chain walked upwards from a clean latent -----------------------------------------------------------
    @torch.no_grad()
    @_lib.with_planes
    def run_invert(self, z0, k, cond, uncond=None, *, first_stage=0, log_every_t=100, callback=None):
        """DDIM's deterministic encoder: every stage s >= first_stage starts from the clean latent z0 (B, C, H, W) -- the earlier stages'
        channels clean, its own window [a_s, e_s) to be noised: the state its denoiser was trained on -- and runs the FIRST k rows of the
        ascending table, x' = c0 x + c1 eps on the window (frido_invert_step), eps at ddim_timesteps[i].  The stages do not depend on one
        another: no hand-off, every stage reads z0.  One captured body per stage ([evaluation, update, +1]) replayed in units of up to
        GRAPH_STEPS; z0 and k are device state or loop bounds, so every z0 / k / guidance scale replays the same graphs.  No noise is
        drawn.  Returns (x_inv NCHW: z0's bits below first_stage, every other window its stage's inverted state -- what
        run(edit=EditSpec(init="noise"), x_T=x_inv) starts its last k rows from --, {"x_inter": [z0, logged states ...]})."""
        assert self.kind == "invert", "run_invert() is the inversion engine's loop"
        assert 1 <= k <= self.n_steps and 0 <= first_stage < self.num_stage, (k, first_stage)
        B, C, H, W = self.B, self.C, self.H, self.W
        o = SimpleNamespace(callback=callback, img_callback=None)
        logged = logged_at(k, log_every_t)
        with own_stream(self, self.dev) as sp:
            ctx = self._context(cond, uncond)
            self.cfg_dev.fill_(self.cfg_scale)
            z = z0.to(self.dev, torch.float32).contiguous()
            assert z.shape == (B, C, H, W), (tuple(z.shape), (B, C, H, W))
            if not hasattr(self, "z0"):
                self.z0 = torch.zeros_like(self.x)
            _relayout(self.b, sp, z, self.z0, B, H * W, C, 0)
            out, inter = z.clone(), {"x_inter": [z.clone()]}
            t_loop = torch.from_numpy(self.t_loop.astype(np.int64)).to(self.dev)
            for s in range(first_stage, self.num_stage):
                a, e = sum(self.embed[:s]), sum(self.embed[:s + 1])
                self.x.copy_(self.z0)
                self._bind_stage(s, ctx, t_loop, sp)

                def log(i, e=e):
                    if callback:
                        callback(i)
                    if logged(i):
                        inter["x_inter"].append(self._to_nchw(self.x, sp)[:, :e])
                key = ("invert", s)
                self._body(key, sp, lambda: [self._eval_ops(s), self._update_op(s), 1])
                self._replay(key, self._unit_steps(o, GRAPH_STEPS), logged, sp, after_unit=log, n=k)
                out[:, a:e] = self._to_nchw(self.x, sp)[:, a:e]       # plumbing: the stage's window into the result
        return out, inter

    # ---- editing: img2img start and keep-mask inpainting in DDIM's loop ---------------------------------------------------------
    def _bind_edit(self, ed, sp):
        """This run's clean latent, stage masks and q_sample coefficients into the engine's fixed buffers (the captured bodies read them:
        another z0 / mask replays the same graphs).  qtab row r = {sqrt_alphas_cumprod[t], sqrt_one_minus_alphas_cumprod[t]} at the chain's
        timestep of row r, gathered from the model's own float32 buffers."""
        B, C, H, W = self.B, self.C, self.H, self.W
        if not hasattr(self, "z0"):
            self.z0 = torch.zeros_like(self.x)
            self.qtab = torch.zeros(self.n_steps, 2, dtype=torch.float32, device=self.dev)
            self.masks = [torch.zeros(B, H * W, dtype=torch.float32, device=self.dev) for _ in range(self.num_stage)]
        z = ed.z0.to(self.dev, torch.float32).contiguous()
        assert z.shape == (B, C, H, W), (tuple(z.shape), (B, C, H, W))
        _relayout(self.b, sp, z, self.z0, B, H * W, C, 0)
        t = torch.from_numpy(self.t_loop.astype(np.int64))
        sa, sb = (v.detach().to("cpu", torch.float32)[t] for v in (ed.sqrt_ac, ed.sqrt_1mac))
        self.qtab.copy_(torch.stack((sa, sb), dim=1))
        if ed.masks is not None:
            assert len(ed.masks) == self.num_stage
            for dst, m in zip(self.masks, ed.masks):
                assert m.shape == (B, 1, H, W), (tuple(m.shape), (B, 1, H, W))
                dst.copy_(m.to(self.dev, torch.float32).reshape(B, H * W))

    def _blend_op(self, s, window, masked, noise=None, clean=False):
        """(kind name, fields) of the editing blend on the engine's state: x <- q * m + (1 - m) * x on the channel window, q = q_sample(z0) at
        the device step counter's row (clean: q = z0).  masked: stage s's mask, else m = 1.  noise: None -- Philox keyed by the device
        {seed, sample0}, draw = row + 1, stream EDIT_RNG_STREAM + s -- or (address, channels) of a host tape read by step index."""
        kw = dict(x=self.x.data_ptr(), z0=self.z0.data_ptr(), mask=self.masks[s].data_ptr() if masked else None, B=self.B, HW=self.H * self.W,
                  Cx=self.C, c0=window[0], c1=window[1], clean=int(clean))
        if not clean:
            kw.update(qtab=self.qtab.data_ptr(), step=self.step.data_ptr())
            if noise is not None:
                kw.update(noise=noise[0], noise_stride=self.B * self.H * self.W * noise[1], noise_C=noise[1])
            else:
                kw.update(rng_dev=self.rng.data_ptr(), rng_stream=EDIT_RNG_STREAM + s)
        return "FRIDO_OP_KEEP_BLEND", kw

    def _edit_stage(self, s, sp, o):
        """One stage of an edit: the last o.n rows of DDIM's chain (the device counter starts at row0 = n_steps - o.n) with the blends of
        csrc/edit.hip around them.
          init "z0": the stage starts from q_sample(z0) on its window at the first row (one unmasked blend; frido.py:302-318 with
                     ch_start: earlier stages clean, the stage's own channels noised -- the state the denoiser was trained on);
          a mask:    before EVERY model evaluation (ddim.py:158-161) x <- q_sample(z0, t) * m + (1 - m) * x on the window: the step body is
                     [blend, evaluation, update, +1].  Under init "z0" step 0 runs the plain body: its state already is that draw;
          reimpose:  after the last step, before the hand-off, z0 itself goes back under the mask (a noise-free blend).
          blend "reference": the window is [0, e_s), the frozen channels included (ddim.py:160-161 read literally).
        Host noise ("torch" / a tape) is drawn per stage in the reference's order -- the start draw, then per step the blend's draw
        (q_sample's randn_like), then the update's -- each (B, e_s, H, W), and uploaded to two tapes read by step index."""
        ed, n, row0 = o.edit, o.n, o.row0
        a, e = sum(self.embed[:s]), sum(self.embed[:s + 1])
        window = (a, e) if ed.blend == "stage" else (0, e)
        masked, start, tape = ed.masks is not None, ed.init == "z0", o.draw is not None
        noise = bnoise = None
        if tape:
            shape, blends, updates = (self.B, e, self.H, self.W), [], []
            first = o.draw(shape) if start else None
            for i in range(n):
                blends.append(o.draw(shape) if masked and not (start and i == 0) else first if i == 0 and start else torch.zeros(shape))
                updates.append(o.draw(shape))
            noise = self._upload_noise(s, updates, row0)
            if start or masked:
                bnoise = self._upload_noise(s, blends, row0, key=("blend", s))
        else:
            self.rng.copy_(torch.tensor([o.seed, o.sample0], dtype=torch.int64))
        log = lambda i: self._log(s, i, sp, o)
        if start:
            self._prog([self._blend_op(s, window, False, bnoise)]).run(sp)
        # blend "reference" rewrites the frozen channels in every step, and the stage's hoisted invariants (`pre`: the SPADE maps) are
        # computed from them: its bodies recompute `pre` in front of every evaluation
        ref = ed.blend == "reference"
        form, pre = ("_tape" if tape else "") + ("_ref" if ref else ""), [list(self.stages[s].pre.ops)] if ref else []
        key = plain = ("ddim" + form, s)
        self._body(plain, sp, lambda: pre + [self._eval_ops(s), self._update_op(s, noise), 1])
        i0 = 0
        if masked:
            key = ("edit" + form, s)
            self._body(key, sp, lambda: [self._blend_op(s, window, True, bnoise)] + pre + [self._eval_ops(s), self._update_op(s, noise), 1])
            if start:
                self._go(self.graphs[plain], sp)
                log(0)
                i0 = 1
        self._replay(key, self._unit_steps(o, GRAPH_STEPS), logged_at(n, o.log_every_t), sp, after_unit=log, n=n, i0=i0)
        if masked and ed.reimpose:
            self._prog([self._blend_op(s, window, True, clean=True)]).run(sp)

    def _plms_stage(self, s, sp, o):
        """plms.py:156-194,285-303: Heun-style first step (two denoiser calls), then Adams-Bashforth 2/3/4.  Two step bodies per stage serve
        every step: `first` = [forward, save x, update with e_t (eps -> ring slot 0), step+1, forward at (x_prev, t_next), step-1, restore x,
        update with (e_t + e_next)/2, step+1]; `body` = [forward, update with the ring history selected by the device step counter, step+1].
        eta == 0 (plms.py:25-26), so no noise enters the update and the same bodies serve the philox / torch / tape modes.
        With a score corrector (plms.py:236-238, inside every model evaluation) the same op sequences run eagerly with the hook after each
        forward; the corrected eps is what enters the history ring (plms.py:175-177 appends get_model_output's result)."""
        plan, n = self.stages[s], self.n_steps
        self.rng.copy_(torch.tensor([o.seed, o.sample0], dtype=torch.int64))
        nbytes = self.x.numel() * 4
        corrector = o.score_corrector is not None
        ev = lambda: self._eval_ops(s)
        upd = lambda mode: self._update_op(s, hist_mode=mode, no_cfg=corrector)
        save = ("FRIDO_OP_COPY", dict(src=self.x.data_ptr(), dst=self.x_save.data_ptr(), n=nbytes))
        restore = ("FRIDO_OP_COPY", dict(src=self.x_save.data_ptr(), dst=self.x.data_ptr(), n=nbytes))
        ahead, back = ([1], [-1]) if n > 1 else ([], [])        # t_next for the second evaluation (plms.py:164-166)
        log = lambda i: self._log(s, i, sp, o)

        def draws(i, unit):
            # eta == 0: the reference still draws (and discards) noise for every update; keep a replayed stream in step
            if o.draw is not None:
                for _ in range(2 if i == 0 else 1):
                    nz = o.draw((self.B, sum(self.embed[:s + 1]), self.H, self.W))
                    if o.noise_dropout > 0.:
                        torch.nn.functional.dropout(nz, p=o.noise_dropout)      # (plms.py get_x_prev_and_pred_x0: the mask draw consumes generator state)
        if corrector:       # step 0 needs the hook twice, inside what is one body otherwise: a loop of its own
            first_a, first_b, body = self._prog([save, upd(1)] + ahead), self._prog(back + [restore, upd(3), 1]), self._prog([upd(1), 1])
            for i in range(n):
                draws(i, 1)
                plan.step.run(sp)
                self._corrected_eps(s, sp, self.t_loop[i], o)
                if i == 0:
                    first_a.run(sp)
                    plan.step.run(sp)
                    self._corrected_eps(s, sp, self.t_loop[min(1, n - 1)], o)
                    first_b.run(sp)
                else:
                    body.run(sp)
                log(i)
            return
        first = self._body(("plms_first", s), sp, lambda: [ev(), save, upd(1)] + ahead + [ev()] + back + [restore, upd(3), 1])
        self._body(("plms_body", s), sp, lambda: [ev(), upd(1), 1])
        self._replay(("plms_body", s), 1, None, sp, before_unit=draws, after_unit=log, first=first)

    # ---- ancestral (DDPM) loop ---------------------------------------------------------------------------
    @torch.no_grad()
    @_lib.with_planes
    def run_ancestral(self, cond, *, x_T=None, noise="torch", seed=0, sample0=0, log_every_t=100, callback=None, img_callback=None,
                      temperature=1.0, noise_dropout=0.0, score_corrector=None, corrector_kwargs=None, model=None, collect="img"):
        """frido.py:1366-1418 (p_sample_loop; collect="img") / :1308-1363 (progressive_denoising; collect="x0"): for every stage, t = T - 1 ... 0,
        one ancestral update of the FULL latent -- no hand-off between the stages, x_T (when given) is the start of stage 0.
        noise: "torch" draws from torch's CPU generator in the reference's order (x_T, then per step one full-shape randn -- t = 0 included --
        and, with noise_dropout, its keep mask); a callable shape -> tensor replays a tape the same way; "philox" draws in the kernel, keyed
        by (seed, global sample index, num_timesteps - t, stage) -- p_sample's key, so one p_sample call reproduces the loop's draw at that
        (t, stage) whatever the chain length.  temperature: a float, or the reference's per-timestep list (host noise only: the
        product noise * temperature[t] is formed on the host, where the reference forms it).  Captured step bodies are replayed in units
        of up to GRAPH_STEPS steps; a step whose result is logged ends its unit; callbacks make every unit one step long; a score corrector
        runs forward program, hook and update kernel eagerly.  Returns (img NCHW, list of logged tensors)."""
        n = self.n_steps
        if noise_dropout > 0. and noise == "philox":
            raise NotImplementedError("noise_dropout draws its keep mask from torch's generator: use noise='torch' (or a recorded tape)")
        draw = self._host_draw(noise)
        if isinstance(temperature, (list, tuple)):
            if draw is None:
                raise NotImplementedError("a per-timestep temperature list needs host noise (noise='torch' or a tape): the Philox form multiplies in the kernel by one scalar")
            temps = [float(v) for v in temperature]
            assert len(temps) >= n, "temperature: one entry per timestep"
        else:
            temps = [float(temperature)] * n
            assert draw is not None or float(temperature) == self.temperature, "the Philox form bakes its temperature into the engine"
        o = SimpleNamespace(draw=draw, seed=seed, sample0=sample0, log_every_t=log_every_t, callback=callback, img_callback=img_callback,
                            noise_dropout=float(noise_dropout), score_corrector=score_corrector, corrector_kwargs=dict(corrector_kwargs or {}),
                            model=model, cond=cond, temps=temps, collect=collect)
        with own_stream(self, self.dev) as sp:
            ctx = self._context(cond)
            self._init_x(x_T, draw, seed, sample0, sp)
            o.inter = [self._to_nchw(self.x, sp)] if collect == "img" else []
            t_loop = torch.from_numpy(self.t_loop.astype(np.int64)).to(self.dev)
            self.rng.copy_(torch.tensor([seed, sample0], dtype=torch.int64))
            for s in range(self.num_stage):
                self._bind_stage(s, ctx, t_loop, sp)
                self._ddpm_stage(s, sp, o)
            out = self._to_nchw(self.x, sp)
        return out, o.inter

    def _ddpm_stage(self, s, sp, o):
        plan, n = self.stages[s], self.n_steps
        B, C, H, W = self.B, self.C, self.H, self.W
        tape = o.draw is not None
        if tape and self.tape is None:
            self.tape = torch.empty(self.unit, B, H, W, C, dtype=torch.float32, device=self.dev)
        noise = (self.tape.data_ptr(), C) if tape else None
        update = lambda: [self._update_op(s, noise), 1] + ([("FRIDO_OP_STEP_ADD", dict(step=self.step_c.data_ptr(), delta=1))] if tape else [])
        logged = logged_at(n, o.log_every_t)          # frido.py:1409: i % log_every_t == 0 or i == timesteps - 1, i = t

        def upload(i, unit):
            if tape:
                rows = []
                for j in range(i, i + unit):
                    nz = torch.as_tensor(o.draw((B, C, H, W)), dtype=torch.float32) * o.temps[n - 1 - j]                      # frido.py:1286
                    rows.append(torch.nn.functional.dropout(nz, p=o.noise_dropout) if o.noise_dropout > 0. else nz)         # frido.py:1288-1289
                self.tape[:unit].copy_(torch.stack(rows).permute(0, 1, 3, 4, 2))                                           # plumbing: layout + H2D
                self.coef_c[:unit].copy_(self.coef[self.row0 + i:self.row0 + i + unit])
                self.step_c.zero_()

        def after(i):
            t = n - 1 - i
            if logged(i):
                o.inter.append(self._to_nchw(self.x if o.collect == "img" else self.pred_x0, sp))
            if o.callback:
                o.callback(t)
            if o.img_callback:
                o.img_callback(self._to_nchw(self.x, sp), t)
        if o.score_corrector is not None:
            upd = self._prog(update())
            for i in range(n):
                upload(i, 1)
                plan.step.run(sp)
                self._corrected_eps(s, sp, self.t_loop[i], o)
                upd.run(sp)
                after(i)
            return
        key = ("ddpm_tape" if tape else "ddpm", s)
        self._body(key, sp, lambda: [self._eval_ops(s)] + update())
        self._replay(key, self._unit_steps(o, self.unit), logged, sp, before_unit=upload, after_unit=after)


class DecoderRuntime(_Runtime):
    def __init__(self, module, vq_cfg, device, precision=None):
        super().__init__(module, vq_cfg, device, precision)
        self.graphs = {}         # reconstruct(): (B, H, W, aux) -> the captured encode + loss + decode graph
        self.graph_captures = 0

    U8_MODES = {False: 0, None: 0, True: 1, "np": 1, "pil": 2}

    def _per_scale(self, factors):
        """A per-scale factor list as the tuple of floats the plan keys hold; None: all ones."""
        return tuple(float(v) for v in (factors if factors is not None else [1.0] * len(self.cfg["embed_dim"])))

    def _dec(self, B, h, w, Ct, inv_scale, forced, u8):
        """(latent state [B][h * w][Ct], VQ decode plan) of one latent shape: the whole-latent decode and the patch-wise decode of crops of
        that shape share it."""
        inv = self._per_scale(inv_scale)
        key = (B, h, w, inv, forced, u8)
        if key not in self.plans:
            z_state = torch.zeros(B, h * w, Ct, dtype=torch.float32, device=self.device)
            self.plans[key] = (z_state, VQDecodePlan(self.b, self.cfg["ddconfig"], self.cfg["embed_dim"], self.cfg["n_embed"], B=B, h=h, w=w,
                                                      z_state=z_state, inv_scale=inv, forced=forced, u8_mode=u8))
        return self.plans[key]

    def _enc(self, B, Cin, H, W, scale):
        """(input buffer (B, Cin, H, W), pre-quant encode plan) of one image shape, shared like _dec's."""
        sc = self._per_scale(scale)
        key = ("enc", B, H, W, sc)
        if key not in self.plans:
            x_in = torch.zeros(B, Cin, H, W, dtype=torch.float32, device=self.device)
            self.plans[key] = (x_in, VQEncodePlan(self.b, self.cfg, B=B, H=H, W=W, x_in=x_in, scale=sc))
        return self.plans[key]

    @_lib.with_planes
    def decode(self, z, inv_scale=None, return_code=False, to_uint8=False, force_codes=None):
        """z (B, Ctot, h, w) NCHW latent -> image (B, 3, H, W); inv_scale: per-scale multiplier (1/scale_factor).
        to_uint8: True / "np" -> the (B, H, W, 3) uint8 array of scripts/sample_diffusion.py:115-121 (custom_to_np), "pil" -> the
        pixel bytes of :103-113 (custom_to_pil's truncating conversion), written by the LAST conv's epilogue (r04: no f32
        image, 4x less to gather / write)."""
        B, Ct, h, w = z.shape
        u8 = self.U8_MODES[to_uint8]
        st = current_stream_ptr(self.device)
        z_state, plan = self._dec(B, h, w, Ct, inv_scale, force_codes is not None, u8)
        if force_codes is not None:      # test hook: decode the given per-scale code maps instead of the argmin's
            for dst, src in zip(plan.force_idx, force_codes):
                dst.copy_(torch.as_tensor(src, dtype=torch.int64).reshape(-1))
        zc = z.contiguous().float()
        _relayout(self.b, st, zc, z_state, B, h * w, Ct, 0)
        plan.prog.run(st)
        if u8:
            out = plan.out_u8.view(B, plan.H, plan.W, plan.a.out_ch).clone()
        else:
            out = torch.empty(B, plan.a.out_ch, plan.H, plan.W, dtype=torch.float32, device=self.device)
            _relayout(self.b, st, plan.out_nhwc, out, B, plan.H * plan.W, plan.a.out_ch, 1)
        return (out, [i.view(B, -1) for i in plan.idx]) if return_code else out

    @_lib.with_planes
    def encode(self, x, scale=None):
        """x (B, 3, H, W) NCHW image -> pre-quantisation latent (B, sum(embed), H/f, W/f); `scale` (per scale) folds
        get_first_stage_encoding's multiply in."""
        x_in, plan = self._enc(*x.shape, scale)
        x_in.copy_(x)            # plumbing: D2D copy into the plan's fixed input buffer
        plan.prog.run(current_stream_ptr(self.device))
        return plan.out.clone()

    # ---- the MS-VQGAN as a model of its own (MSFPNVQModel: taming/models/msvqgan.py:116-186, 266-309) ----
    def _encq(self, B, Cin, H, W):
        """(input buffer, quantised encode plan, its loss state) of one image shape."""
        key = ("encq", B, H, W)
        if key not in self.plans:
            from .vqloss import CommitLoss
            embed = self.cfg["embed_dim"]
            x_in = torch.zeros(B, Cin, H, W, dtype=torch.float32, device=self.device)
            plan = VQEncodePlan(self.b, self.cfg, B=B, H=H, W=W, x_in=x_in, scale=[1.0] * len(embed), quantized=True)
            loss = CommitLoss(plan, embed, self.cfg.get("quant_beta", 0.25), self.cfg.get("legacy", True), self.device)
            self.plans[key] = (x_in, plan, loss)
        return self.plans[key]

    def _decq(self, Bs, h, w, groups, u8, src=None):
        """(input buffer, decode-from-quant plan); src: another plan's quant tensor to read instead of an input buffer of its own."""
        key = ("decq", Bs, h, w, groups, u8, None if src is None else src.data_ptr())
        if key not in self.plans:
            embed = self.cfg["embed_dim"]
            q_in = src if src is not None else torch.zeros(Bs, sum(embed), h, w, dtype=torch.float32, device=self.device)
            self.plans[key] = (q_in, VQDecodeQuantPlan(self.b, self.cfg["ddconfig"], embed, Bs=Bs, h=h, w=w, quant_src=q_in,
                                                       groups=groups, u8_mode=u8))
        return self.plans[key]

    @_lib.with_planes
    def encode_quant(self, x):
        """x (B, 3, H, W) NCHW image -> (quant (B, sum(embed), H/f, W/f): the quantised multi-scale latent, channels [fine .. coarse],
        emb_loss: 0-d f32, [idx_s]: int64 [B * h_s * w_s] per scale, coarse first) -- device tensors; the encode program and the loss
        launcher go out on the current stream and nothing waits for them."""
        from .vqloss import launch_vq_commit_loss
        B, Cin, H, W = x.shape
        x_in, plan, loss = self._encq(B, Cin, H, W)
        st = current_stream_ptr(self.device)
        x_in.copy_(x)            # plumbing: D2D copy into the plan's fixed input buffer
        plan.prog.run(st)
        launch_vq_commit_loss(loss.desc, st)
        return plan.quant.clone(), loss.total.clone(), [i.clone() for i in plan.idx]

    @_lib.with_planes
    def decode_quant(self, quant, to_uint8=False, groups=None):
        """quant (B, sum(embed), h, w) NCHW, already quantised, channels [fine .. coarse] -> image (B, 3, H, W): post_quant_conv + decoder,
        no VQ lookup.  groups: channel ranges (c0, c1) -- the result is (len(groups) * B, 3, H, W), entries g * B ... decoded from quant with
        everything outside group g's range zeroed, all as one batch.  to_uint8 as in decode()."""
        B, Ct, h, w = quant.shape
        assert Ct == sum(self.cfg["embed_dim"]), f"the quantised latent has {sum(self.cfg['embed_dim'])} channels, got {Ct}"
        u8 = self.U8_MODES[to_uint8]
        groups = None if groups is None else tuple(tuple(int(v) for v in g) for g in groups)
        q_in, plan = self._decq(B, h, w, groups, u8)
        q_in.copy_(quant)
        plan.prog.run(current_stream_ptr(self.device))
        return (plan.out_u8 if u8 else plan.out).clone()

    def aux_groups(self):
        """Channel ranges of MSFPNVQModel.forward's three decodes (msvqgan.py:168-177): everything, the last embed_dim[-1] channels, the
        first embed_dim[-1] channels."""
        embed = self.cfg["embed_dim"]
        Ct = sum(embed)
        return ((0, Ct), (Ct - embed[-1], Ct), (0, embed[-1]))

    @_lib.with_planes
    def reconstruct(self, x, aux=False, use_graph=True):
        """MSFPNVQModel.forward (msvqgan.py:166-186): encode program -> codebook loss -> decode program as ONE captured graph per
        (B, H, W, aux), replayed on later batches; quant stays on the device between the halves.  aux: the three decodes of :168-177 as one
        decoder program at batch 3B.  Returns (dec (B or 3B, 3, H, W), quant, emb_loss, [idx_s])."""
        B, Cin, H, W = x.shape
        x_in, enc, loss = self._encq(B, Cin, H, W)
        h, w = enc.quant.shape[2:]
        _, dec = self._decq(B, h, w, self.aux_groups() if aux else None, 0, src=enc.quant)
        with own_stream(self, self.device) as sp:
            x_in.copy_(x)
            key = ("rec", B, H, W, bool(aux), bool(use_graph))
            if key not in self.graphs:
                prog = Prog(self.device, self.nsplit)
                prog.ops = list(enc.prog.ops) + [_lib.op_of("FRIDO_OP_VQ_COMMIT_LOSS", loss.desc)] + list(dec.prog.ops)
                prog.keep = [enc, loss, dec]
                self.graphs[key] = prog.capture(sp) if use_graph else prog
                self.graph_captures += 1
            g = self.graphs[key]
            g.launch(sp) if use_graph else g.run(sp)
            return dec.out.clone(), enc.quant.clone(), loss.total.clone(), [i.clone() for i in enc.idx]

    # ---- patch-wise mode (FridoDiffusion.split_input_params with patch_distributed_vq, frido.py:840-877, 963-993) ----
    @_lib.with_planes
    def decode_patches(self, z, geo, inv_scale=None, to_uint8=False):
        """z (B, Ctot, h, w) NCHW latent -> image (B, 3, h * vqf, w * vqf): the latent's crops (patching.PatchGeometry `geo`, DECODE mode) are
        decoded as ONE batch of B * L by the decode plan (f32 NHWC crops out of its last conv) and folded at image resolution; with
        to_uint8 the fold kernel writes the (B, H, W, 3) uint8 image through the last conv's two conversions."""
        from .patching import launch_fold
        B, Ct = z.shape[:2]
        _, _, kh, kw, _, _ = geo.src
        H, W, kho, kwo, _, _ = geo.out
        u8 = self.U8_MODES[to_uint8]
        st = current_stream_ptr(self.device)
        z_state, plan = self._dec(B * geo.L, kh, kw, Ct, inv_scale, False, 0)
        if (plan.H, plan.W) != (kho, kwo):
            raise ValueError(f"split_input_params['vqf'] = {kho // kh} does not match the first stage, which decodes {kh} x {kw} latents to "
                             f"{plan.H} x {plan.W} images")
        Co = plan.a.out_ch
        _unfold_nhwc(self.b, st, geo, z.contiguous().float(), crops=z_state)
        plan.prog.run(st)
        if u8:
            img = torch.empty(B, H, W, Co, dtype=torch.uint8, device=self.device)
            launch_fold(geo.fold_desc(plan.out_nhwc.data_ptr(), None, B, Co, out_u8=img.data_ptr(), u8_mode=u8), st)
            return img
        return _fold_nchw(self.b, st, geo, plan.out_nhwc, B, Co)

    @_lib.with_planes
    def encode_patches(self, x, geo):
        """x (B, 3, H, W) NCHW image -> pre-quantisation latent (B, sum(embed), H / vqf, W / vqf): image crops (`geo`, ENCODE mode) encoded
        as one batch, folded at latent resolution."""
        B, Cin = x.shape[:2]
        _, _, kh, kw, _, _ = geo.src
        _, _, kho, kwo, _, _ = geo.out
        x_in, plan = self._enc(B * geo.L, Cin, kh, kw, None)
        if tuple(plan.out.shape[2:]) != (kho, kwo):
            raise ValueError(f"split_input_params['vqf'] = {kh // kho} does not match the first stage, which encodes {kh} x {kw} images to "
                             f"{tuple(plan.out.shape[2:])} latents")
        patch_unfold(self.b, geo, x.contiguous().float(), out=x_in)
        plan.prog.run(current_stream_ptr(self.device))
        return patch_fold(self.b, geo, plan.out, B)
