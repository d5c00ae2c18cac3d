"""DDIMSampler / PLMSSampler with the reference's constructor and `.sample(...)` signature
(frido/models/diffusion/ddim.py:11-114, plms.py:11-114), driving the HIP SamplerEngine; DPMSolverSampler, which the reference does not
have (upstream latent-diffusion ships one with this signature): DPM-Solver++(2M) on the same engine.

Noise: the reference draws x_T and one torch.randn per update from torch's global generator of the device it runs on.
With noise="torch" (default) the same draws are made from the HOST generator in the same order and uploaded, so a run after
torch.manual_seed(s) consumes exactly the noise stream of a reference run ON CPU with that seed (a reference run on a GPU
draws from that device's generator, a different stream); noise="philox" uses the device counter RNG keyed by
(seed, global sample index) instead (no host involvement, shard-invariant).
"""
import collections

import numpy as np
import torch

ENGINE_CACHE_SIZE = 4      # compiled SamplerEngines kept per denoiser (each owns per-stage plans, buffers and graphs)

from . import schedules
from ._lib import FridoHipError
from .engine import lru_entry


def check_conditioning(unet, conditioning, batch_size, name="conditioning"):
    """What every sampling loop (DDIM / PLMS `sample`, the ancestral loops) asks of its conditioning before it plans anything; returns
    the engine-cache mode: the context length, "labels" or "uncond"."""
    has_ctx = getattr(unet, "use_spatial_transformer", True)
    labels = getattr(unet, "num_classes", None) is not None
    if isinstance(conditioning, dict):
        raise NotImplementedError("dict conditionings ('concat' / 'hybrid'): pass the cross-attention conditioning tensor or the class labels")
    if conditioning is None:
        if has_ctx:
            raise NotImplementedError("cross-attention conditioning tensor required")
        if labels:
            raise ValueError(f"a class-conditional denoiser needs its labels as `{name}`")
        return "uncond"
    if not has_ctx and not labels:
        raise ValueError(f"this denoiser takes neither a context nor class labels: pass {name}=None")
    if conditioning.shape[0] != batch_size:
        # the reference only prints a warning here (ddim.py:87-93) and then fails (or silently broadcasts) inside the
        # denoiser; a mismatched batch is never what the caller meant
        raise ValueError(f"Got {conditioning.shape[0]} conditionings but batch-size is {batch_size}")
    if labels:
        want = (batch_size,) if unet.use_embed else (batch_size, unet.num_classes)
        if tuple(conditioning.shape) != want:
            raise ValueError(f"class labels of shape {tuple(conditioning.shape)}: this denoiser takes {want}")
    return conditioning.shape[1] if has_ctx else "labels"


def cached_engine(rt, key, make):
    """The denoiser runtime's least-recently-used cache of SamplerEngines, shared by every sampler kind: `make()` builds a missing one.
    An evicted engine owns its plans' persistent buffers (Builder.persist_scope) and graphs, so its HBM is released with it -- the
    activation pool is shared and reused."""
    return lru_entry(rt.__dict__.setdefault("_sampler_engines", collections.OrderedDict()), key, ENGINE_CACHE_SIZE, make)


def edit_steps(S, t_start=None, strength=None):
    """How many of the S steps an edit runs: exactly one of t_start (the integer itself, in [1, S]) and strength
    (clamp(int(strength * S), 1, S)) is given."""
    if (t_start is None) == (strength is None):
        raise ValueError("edit: give exactly one of t_start (steps to run) and strength (the fraction of the S steps)")
    if strength is not None:
        return min(max(int(strength * S), 1), S)
    if isinstance(t_start, bool) or not isinstance(t_start, (int, np.integer)) or not 1 <= t_start <= S:
        raise ValueError(f"edit: t_start={t_start!r} must be an integer in [1, {S}]")
    return int(t_start)


COMPOSE_MAX = 7            # entries of `compose=`: with the main conditioning, the 8 slots of frido_guidance_compose


def check_compose(who, model, conditioning, unconditional_conditioning, scale, compose, guidance_rescale, score_corrector=None):
    """What `compose=` / `guidance_rescale=` ask before anything is planned.  Returns None for a call without them -- today's path -- or
    (conditionings, weights, phi): the main conditioning first with weight `scale`, then the entries of `compose` in their order."""
    if compose is None and isinstance(guidance_rescale, (int, float)) and guidance_rescale == 0:
        return None
    no = lambda what: NotImplementedError(f"{who}: {what} is not built for composed guidance (compose= / guidance_rescale=)")
    from . import patching
    if patching.params_of(model) is not None:
        raise patching.refuse(f"{who}: composed guidance (compose= / guidance_rescale=)")
    if score_corrector is not None:
        raise no("score_corrector")
    entries = list(compose) if compose is not None else []
    if isinstance(compose, dict) or any(not isinstance(e, (tuple, list)) or len(e) != 2 for e in entries):
        raise ValueError(f"{who}: compose is a sequence of (conditioning, weight) pairs")
    if isinstance(conditioning, (dict, list)) or isinstance(unconditional_conditioning, (dict, list)) or \
            any(isinstance(c, (dict, list)) for c, _ in entries):
        raise no("a dict / list conditioning")
    if isinstance(guidance_rescale, bool) or not isinstance(guidance_rescale, (int, float, np.integer, np.floating)) or \
            not 0.0 <= float(guidance_rescale) <= 1.0:
        raise ValueError(f"{who}: guidance_rescale={guidance_rescale!r} must be a number in [0, 1]")
    if len(entries) > COMPOSE_MAX:
        raise ValueError(f"{who}: compose holds {len(entries)} entries, at most {COMPOSE_MAX} fit beside the main conditioning")
    if unconditional_conditioning is None or not torch.is_tensor(conditioning):
        raise ValueError(f"{who}: compose= / guidance_rescale= need a conditioning and an unconditional_conditioning (every term is "
                         "measured against the unconditional evaluation)")
    for i, (c, w) in enumerate(entries):
        if not torch.is_tensor(c) or c.shape != conditioning.shape or c.device != conditioning.device or \
                c.is_floating_point() != conditioning.is_floating_point():
            raise ValueError(f"{who}: compose[{i}] must be a tensor like conditioning ({tuple(conditioning.shape)}, "
                             f"{'floating' if conditioning.is_floating_point() else 'integer'}, on {conditioning.device}), got "
                             f"{(tuple(c.shape), c.dtype, str(c.device)) if torch.is_tensor(c) else type(c).__name__}")
    weights = [scale] + [w for _, w in entries]
    for i, w in enumerate(weights):
        if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)) or not np.isfinite(float(w)):
            raise ValueError(f"{who}: weight {w!r} of {'the main conditioning' if i == 0 else f'compose[{i - 1}]'} must be a finite real number")
    if not entries and float(guidance_rescale) == 0.0:
        return None         # an empty composition without rescale is classifier-free guidance: today's path
    return [conditioning] + [c for c, _ in entries], [float(w) for w in weights], float(guidance_rescale)


def _composed_call(comp, conditioning):
    """check_compose's result -> (what SamplerEngine.run takes as cond, the engine key's (ncond, rescale on) or None, run's extra keywords)."""
    if comp is None:
        return conditioning, None, {}
    conds, weights, phi = comp
    return conds, (len(conds), phi != 0.0), dict(weights=weights, phi=phi)


class _SamplerBase:
    KIND = "ddim"

    def __init__(self, model, schedule="linear", **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule

    def register_buffer(self, name, attr):
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if self.KIND == "plms" and ddim_eta != 0:
            raise ValueError("ddim_eta must be 0 for PLMS")
        ac = self.model.alphas_cumprod.detach().float().cpu().numpy()
        assert ac.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        self.ddim_num_steps = ddim_num_steps
        self.ddim_timesteps = schedules.make_ddim_timesteps(ddim_discretize, ddim_num_steps, self.ddpm_num_timesteps)
        sig, al, alp = schedules.make_ddim_sampling_parameters(ac, self.ddim_timesteps, ddim_eta)
        self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev = sig, al, alp
        self.ddim_sqrt_one_minus_alphas = np.sqrt((np.float32(1.0) - al).astype(np.float32))
        self.alphas_cumprod = ac

    def _engine_key(self, B, shape, nctx, S, eta, scale, num_stage, temperature, replica=0, patch=None, solver=None, kind=None, composed=None):
        """The engine-cache key of a call (no device is touched).  composed: None, or (ncond, rescale on) of a call with compose= /
        guidance_rescale= -- appended only then, the way `patch` extends the key: a call without the keywords finds the engine it always
        found.  The weights and the rescale factor are device state, not part of the key."""
        C, H, W = shape
        guided = scale != 1.0 or composed is not None      # a composed engine's scale is one of its weights: every scale shares it
        if solver is None:
            key = (kind or self.KIND, B, C, H, W, nctx, S, float(eta), guided, num_stage, float(temperature), replica)
        else:
            key = (self.KIND, B, C, H, W, nctx, S, guided, num_stage, replica) + solver
        if patch is not None:      # patch-wise mode (model.split_input_params): plans, buffers and graphs of its own
            from .patching import geometry_key
            key += (geometry_key(patch),)
        if composed is not None:
            key += (("compose",) + tuple(composed),)
        return key

    def _engine(self, B, shape, nctx, S, eta, scale, num_stage, temperature, replica=0, patch=None, solver=None, kind=None, composed=None):
        """The cached SamplerEngine of this call.  solver: DPM-Solver++'s (order, skip_type, lower_order_final), part of its engine's key where
        DDIM / PLMS have eta and the temperature; its table is computed from the float64 schedule.  kind: another loop of this sampler
        ("invert": DDIMSampler.invert), with engines -- plans, tables, graphs -- of its own under its own key.  composed: (ncond, rescale on)
        of a call with compose= / guidance_rescale=, an engine of its own (SamplerEngine(ncond=, rescale=))."""
        kind = kind or self.KIND
        from .runtime import SamplerEngine
        unet = self.model.model.diffusion_model
        rt = unet.runtime()
        C, H, W = shape
        key = self._engine_key(B, shape, nctx, S, eta, scale, num_stage, temperature, replica, patch, solver, kind, composed)
        if solver is None:
            more, ac = dict(temperature=temperature, patch=patch), self.model.alphas_cumprod.detach().float()
        else:
            more, ac = dict(zip(("order", "skip_type", "lower_order_final"), solver)), self.model.alphas_cumprod.detach().double()
        if composed is not None:
            more.update(ncond=composed[0], rescale=composed[1])
        eng = cached_engine(rt, key, lambda: SamplerEngine(
            rt.builder_for(replica), unet.cfg, B=B, C=C, H=H, W=W, nctx=nctx if isinstance(nctx, int) else 0, S=S, eta=eta, kind=kind,
            alphas_cumprod=ac.cpu().numpy(), embed_dim=self.model.embed_dim_list, cfg_scale=scale, num_stage=num_stage, **more))
        eng.cfg_scale = float(scale)      # read from a device scalar by the captured step bodies: one graph, any scale
        return eng

    def _check_guidance(self, conditioning, unconditional_conditioning, scale, batch_size):
        """What every `sample` asks of its conditioning pair; returns the engine-cache mode: the context length, or which conditioning mode
        the plans were built for (check_conditioning)."""
        unet = getattr(getattr(self.model, "model", None), "diffusion_model", None)
        mode = check_conditioning(unet, conditioning, batch_size)
        if conditioning is None:
            if scale != 1.:
                raise ValueError("classifier-free guidance needs a conditioning")
        else:
            if unconditional_conditioning is not None and unconditional_conditioning.shape != conditioning.shape:
                raise ValueError(f"unconditional_conditioning {tuple(unconditional_conditioning.shape)} must match "
                                 f"conditioning {tuple(conditioning.shape)}")
            if not conditioning.is_cuda:
                raise FridoHipError("sample(): conditioning must live on the MI355X (there is no CPU path)")
        return mode

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, num_stage=1, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, noise="torch", seed=0, sample0=0,
               replica=0, compose=None, guidance_rescale=0., **kwargs):
        """compose (a sequence of up to 7 (conditioning_i, weight_i)) / guidance_rescale (phi in [0, 1]): composed guidance, see
        check_compose and SamplerEngine -- eps = e_u + s (e_c - e_u) + sum_i w_i (e_i - e_u) with s = unconditional_guidance_scale the
        weight of `conditioning`, terms added in that order, then (phi > 0) scaled per sample by phi sigma(e_c) / sigma(eps) + 1 - phi.
        Both need unconditional_conditioning; split_input_params, score_corrector and dict / list conditionings are refused by name."""
        if mask is not None or x0 is not None:
            # ddim.py:158-161 / plms.py blend `q_sample(x0, ts) * mask + (1 - mask) * img`, but img carries only the channels of the
            # stages reached so far: with num_stage > 1 -- every Frido model -- the reference itself raises a RuntimeError (size
            # mismatch) in stage 0 (full-channel x0) or in stage 1 (stage-0-channel x0); verified against the reference on CPU
            raise NotImplementedError("mask / x0 (inpainting): the reference's blend fails for multi-stage models (shape mismatch between "
                                      "x0 and the per-stage latent, ddim.py:158-161); not provided on the HIP path")
        if quantize_x0:
            raise NotImplementedError("quantize_x0: the reference calls exit() on this option (ddim.py:251-253)")
        # patch-wise mode (frido.py:1076-1152): the samplers inherit it from apply_model; looked up on every call, like the reference's hasattr
        from . import patching
        comp = check_compose(f"{type(self).__name__}.sample", self.model, conditioning, unconditional_conditioning,
                             unconditional_guidance_scale, compose, guidance_rescale, score_corrector)
        patch = patching.params_of(self.model)
        if patch is not None:
            if score_corrector is not None:
                raise patching.refuse("score_corrector")
            patching.check_conditioning(self.model, conditioning)
            patching.check_conditioning(self.model, unconditional_conditioning)
            patching.geometry(patch, shape[1], shape[2], patching.MODEL, None)      # the geometry's own refusals, before anything is planned
        mode = self._check_guidance(conditioning, unconditional_conditioning, unconditional_guidance_scale, batch_size)
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        if unconditional_guidance_scale != 1.:
            assert unconditional_conditioning is not None
        if verbose:
            print(f"Data shape for {self.KIND.upper()} sampling is {(batch_size, *shape)}, eta {eta}")
        self.num_stage = num_stage
        conds, composed, guide = _composed_call(comp, conditioning)

        def go(noise_src):
            # the engine is looked up per attempt: a repeated run (autoplanes: the default plane format saturated) belongs to the
            # denoiser's NEW runtime on the bf16-pair build, with its own plans, buffers and graphs
            eng = self._engine(batch_size, tuple(shape), mode, S, eta, unconditional_guidance_scale, num_stage,
                               temperature, replica, patch, composed=composed)
            return eng.run(conds, unconditional_conditioning, x_T=x_T, noise=noise_src, seed=seed, sample0=sample0,
                           log_every_t=log_every_t, callback=callback, img_callback=img_callback, noise_dropout=noise_dropout,
                           score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, model=self.model, **guide)
        from . import autoplanes
        return autoplanes.run(self.model.model.diffusion_model, go, f"{type(self).__name__}.sample", noise=noise)

    @torch.no_grad()
    def edit(self, S, z0, conditioning=None, *, t_start=None, strength=None, keep_mask=None, init="z0", blend="stage", reimpose=True,
             first_stage=0, num_stage=1, eta=0., x_T=None, temperature=1., unconditional_guidance_scale=1.,
             unconditional_conditioning=None, noise="torch", seed=0, sample0=0, callback=None, img_callback=None, log_every_t=100,
             verbose=True, replica=0, score_corrector=None, noise_dropout=0., compose=None, guidance_rescale=0.):
        """Edit the latent z0 (B, C, H, W) instead of sampling one: the LAST k of the S DDIM steps in every stage from `first_stage` on,
        k = t_start or clamp(int(strength * S), 1, S).  Returns (samples, intermediates) like `sample`.  (Where S does not divide the model's
        timesteps the uniform grid has more than S rows -- 7 at S = 6 of 1000 -- and k still counts from its end.)

        init="z0" (img2img / SDEdit): every stage starts from q_sample of z0 at the chain's first timestep on the stage's own channels --
        Frido's own multi-stage form (frido.py:302-318 with ch_start: earlier stages clean, the stage's channels noised), the state the
        denoiser was trained on.  init="noise": the start is x_T, or a draw as in `sample`.
        keep_mask (B, 1, H, W) in [0, 1], 1 = keep z0 (inpainting): before every denoiser evaluation
        x <- q_sample(z0, t) * m + (1 - m) * x (ddim.py:158-161) with the stage's mask -- the mask's minimum over the stage's
        2^(num_stage - 1 - s) blocks, so a coarse cell is kept only where all of it is; reimpose: after a stage's last step z0 itself is
        put back under the mask.
        blend="stage" (default) blends the stage's own channels [a_s, e_s).  blend="reference" blends [0, e_s), the literal reading of
        ddim.py:160-161 where the reference does run (x_T given, so stage 0 is adopted and stage 1 has x0's channels): it re-noises the
        frozen coarse channels in every step, which the stage's denoiser never saw in training and which the hand-off has already fixed,
        so it is kept to pin the arithmetic and the draw order to the reference, not as the default.
        Stages below first_stage keep the start state's channels (z0's, or x_T's under init="noise").
        noise: "torch" / a tape draw per stage in the reference's order -- the start draw, then per step the blend's draw and the update's
        draw, each (B, e_s, H, W); "philox": keyed by (seed, global sample index), the blend draws on streams of their own.
        compose / guidance_rescale: composed guidance, as in `sample`.
        `sample(mask=, x0=)` stays refused; PLMS / DPM-Solver editing, split_input_params, score_corrector, noise_dropout and dict / list
        conditionings are refused by name."""
        no = lambda what: NotImplementedError(f"{type(self).__name__}.edit: {what} is not built for editing")
        if self.KIND != "ddim":
            raise no(f"{type(self).__name__} (editing runs in DDIM's loop: use DDIMSampler.edit)")
        from . import patching
        if patching.params_of(self.model) is not None:
            raise no("split_input_params (the patch-wise mode)")
        if score_corrector is not None:
            raise no("score_corrector")
        if noise_dropout:
            raise no("noise_dropout")
        if isinstance(conditioning, (dict, list)) or isinstance(unconditional_conditioning, (dict, list)):
            raise no("a dict / list conditioning")
        comp = check_compose(f"{type(self).__name__}.edit", self.model, conditioning, unconditional_conditioning,
                             unconditional_guidance_scale, compose, guidance_rescale)
        k = edit_steps(S, t_start, strength)
        if init not in ("z0", "noise") or blend not in ("stage", "reference"):
            raise ValueError(f"edit: init={init!r} ('z0' or 'noise'), blend={blend!r} ('stage' or 'reference')")
        if not 0 <= first_stage < num_stage:
            raise ValueError(f"edit: first_stage={first_stage} must name one of the {num_stage} stages that run")
        if init == "noise" and keep_mask is None and x_T is None:
            raise ValueError("edit: init='noise' with neither keep_mask nor x_T edits nothing -- that is sample()")
        if init == "z0" and x_T is not None:
            raise ValueError("edit: x_T is the start state of init='noise'; init='z0' starts from z0")
        if not torch.is_tensor(z0) or z0.dim() != 4:
            raise ValueError("edit: z0 is the (B, C, H, W) latent to edit")
        B, shape = z0.shape[0], tuple(z0.shape[1:])
        if keep_mask is not None:
            if not torch.is_tensor(keep_mask) or tuple(keep_mask.shape) != (B, 1) + shape[1:]:
                raise ValueError(f"edit: keep_mask must be {(B, 1) + shape[1:]}, got {tuple(getattr(keep_mask, 'shape', ()))}")
            if keep_mask.device != z0.device:
                raise ValueError(f"edit: keep_mask lives on {keep_mask.device}, z0 on {z0.device}")
        if x_T is not None and tuple(x_T.shape) != (B,) + shape:
            raise ValueError(f"edit: x_T must be {(B,) + shape}, got {tuple(x_T.shape)}")
        mode = self._check_guidance(conditioning, unconditional_conditioning, unconditional_guidance_scale, B)
        if not z0.is_cuda:
            raise FridoHipError("edit(): z0 must live on the MI355X (there is no CPU path)")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        if unconditional_guidance_scale != 1.:
            assert unconditional_conditioning is not None
        if verbose:
            print(f"Data shape for DDIM editing is {(B, *shape)}, eta {eta}, the last {k} of {S} steps")
        self.num_stage = num_stage
        from .runtime import EditSpec, stage_masks
        masks = stage_masks(keep_mask.float(), num_stage) if keep_mask is not None else None
        spec = EditSpec(z0, k, self.model.sqrt_alphas_cumprod, self.model.sqrt_one_minus_alphas_cumprod, masks, init, blend, reimpose, first_stage)
        conds, composed, guide = _composed_call(comp, conditioning)

        def go(noise_src):
            eng = self._engine(B, shape, mode, S, eta, unconditional_guidance_scale, num_stage, temperature, replica, composed=composed)
            return eng.run(conds, unconditional_conditioning, x_T=x_T, noise=noise_src, seed=seed, sample0=sample0,
                           log_every_t=log_every_t, callback=callback, img_callback=img_callback, model=self.model, edit=spec, **guide)
        from . import autoplanes
        return autoplanes.run(self.model.model.diffusion_model, go, f"{type(self).__name__}.edit", noise=noise)

    @torch.no_grad()
    def invert(self, S, z0, conditioning=None, *, t_start=None, strength=None, first_stage=0, num_stage=1,
               unconditional_guidance_scale=1., unconditional_conditioning=None, log_every_t=100, callback=None, verbose=True, replica=0,
               score_corrector=None, compose=None, guidance_rescale=0.):
        """DDIM inversion (DDIM's deterministic encoder; upstream latent-diffusion's DDIMSampler.encode, not in the reference): walk the
        probability-flow ODE UPWARDS from the clean latent z0 (B, C, H, W) through the first k rows of the S-step grid,
        k = t_start or clamp(int(strength * S), 1, S) -- the rows `edit` counts from the chain's end.  Row i, evaluated at
        ddim_timesteps[i], is x' = sqrt(a / p) x + sqrt(a) (sqrt(1 / a - 1) - sqrt(1 / p - 1)) eps with a = ddim_alphas[i],
        p = ddim_alphas_prev[i] (schedules.ddim_inversion_table): the exact inverse of the eta = 0 update of that row for the same eps.
        Every stage from `first_stage` on inverts its own channels [a_s, e_s) from z0[:, :e_s] (earlier stages clean, its window noised:
        what its denoiser reads); the stages do not depend on one another.  Returns (x_inv, {"x_inter": [...]}): x_inv has z0's bits
        below first_stage and every other window at level ddim_alphas[k - 1], where
        `edit(S, z0, c, init="noise", x_T=x_inv, t_start=k, first_stage=f, eta=0)` starts -- with the same conditioning it comes back to
        z0 up to the discretisation error, with another one it edits.  Deterministic: no generator is touched.
        PLMS / DPM-Solver inversion, split_input_params, score_corrector, composed guidance (compose= / guidance_rescale=) and dict / list
        conditionings are refused by name."""
        no = lambda what: NotImplementedError(f"{type(self).__name__}.invert: {what} is not built for inversion")
        if compose is not None or guidance_rescale:
            raise no("composed guidance (compose= / guidance_rescale=)")
        if self.KIND != "ddim":
            raise no(f"{type(self).__name__} (inversion walks DDIM's chain: use DDIMSampler.invert)")
        from . import patching
        if patching.params_of(self.model) is not None:
            raise no("split_input_params (the patch-wise mode)")
        if score_corrector is not None:
            raise no("score_corrector")
        if isinstance(conditioning, (dict, list)) or isinstance(unconditional_conditioning, (dict, list)):
            raise no("a dict / list conditioning")
        k = edit_steps(S, t_start, strength)
        if not 0 <= first_stage < num_stage:
            raise ValueError(f"invert: first_stage={first_stage} must name one of the {num_stage} stages that run")
        if not torch.is_tensor(z0) or z0.dim() != 4:
            raise ValueError("invert: z0 is the (B, C, H, W) latent to invert")
        B, shape = z0.shape[0], tuple(z0.shape[1:])
        mode = self._check_guidance(conditioning, unconditional_conditioning, unconditional_guidance_scale, B)
        if not z0.is_cuda:
            raise FridoHipError("invert(): z0 must live on the MI355X (there is no CPU path)")
        self.make_schedule(ddim_num_steps=S, ddim_eta=0., verbose=verbose)
        if unconditional_guidance_scale != 1.:
            assert unconditional_conditioning is not None
        if verbose:
            print(f"Data shape for DDIM inversion is {(B, *shape)}, the first {k} of {S} steps")
        self.num_stage = num_stage

        def go(_):
            eng = self._engine(B, shape, mode, S, 0.0, unconditional_guidance_scale, num_stage, 1.0, replica, kind="invert")
            return eng.run_invert(z0, k, conditioning, unconditional_conditioning, first_stage=first_stage, log_every_t=log_every_t,
                                  callback=callback)
        from . import autoplanes
        return autoplanes.run(self.model.model.diffusion_model, go, f"{type(self).__name__}.invert")

    def encode(self, x0, c, t_enc, use_original_steps=False, return_intermediates=None, unconditional_guidance_scale=1.0,
               unconditional_conditioning=None, callback=None, **kwargs):
        """Upstream latent-diffusion's argument order for `invert`: t_enc rows of the schedule last made (make_schedule(ddim_num_steps))."""
        if use_original_steps or not hasattr(self, "ddim_num_steps"):
            raise NotImplementedError(f"{type(self).__name__}.encode: call make_schedule(ddim_num_steps) first; use_original_steps (the "
                                      "model's own chain) is not built for inversion")
        return self.invert(self.ddim_num_steps, x0, c, t_start=t_enc, unconditional_guidance_scale=unconditional_guidance_scale,
                           unconditional_conditioning=unconditional_conditioning, callback=callback, **kwargs)


class DDIMSampler(_SamplerBase):
    KIND = "ddim"


class PLMSSampler(_SamplerBase):
    KIND = "plms"


class DPMSolverSampler(_SamplerBase):
    """DPM-Solver++(2M) (Lu et al. 2022: data prediction, multistep): DDIM's `.sample(...)` plus `order` (1 or 2), `skip_type` ("logSNR":
    steps uniform in the log signal-to-noise ratio, snapped to the model's integer timesteps; "time_uniform": DDIM's grid) and
    `lower_order_final` (the last step first-order).  With order=1 and skip_type="time_uniform" it is DDIM at eta = 0.  The solver is
    deterministic: `noise` / `seed` only draw x_T (the host generator in the reference's order, or Philox).  The stages, the hand-off
    between them, an adopted x_T, the intermediates and the callbacks are DDIM's.  What it cannot honour is refused by name."""
    KIND = "dpm"

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, num_stage=1, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, noise="torch", seed=0, sample0=0,
               replica=0, order=2, skip_type="logSNR", lower_order_final=True, compose=None, guidance_rescale=0., **kwargs):
        no = lambda what, why: NotImplementedError(f"DPMSolverSampler: {what} -- {why}")
        if eta != 0:
            raise no(f"eta={eta}", "the multistep solver integrates the probability-flow ODE; it has no stochastic (SDE) variant here")
        if temperature != 1.:
            raise no(f"temperature={temperature}", "no noise enters the update that it could scale")
        if noise_dropout:
            raise no(f"noise_dropout={noise_dropout}", "no noise enters the update that it could drop")
        if score_corrector is not None:
            raise no("score_corrector", "the captured step body has no hook between the denoiser and the update")
        if mask is not None or x0 is not None:
            raise no("mask / x0 (inpainting)", "the reference's own blend fails for multi-stage models (ddim.py:158-161), there is nothing to follow")
        if quantize_x0:
            raise no("quantize_x0", "the reference calls exit() on this option (ddim.py:251-253)")
        from . import patching
        if patching.params_of(self.model) is not None:
            raise patching.refuse("DPMSolverSampler")
        if isinstance(conditioning, (dict, list)) or isinstance(unconditional_conditioning, (dict, list)):
            raise no("dict / list conditionings", "pass the cross-attention conditioning tensor or the class labels")
        comp = check_compose("DPMSolverSampler.sample", self.model, conditioning, unconditional_conditioning, unconditional_guidance_scale,
                             compose, guidance_rescale)
        if order not in (1, 2):
            raise ValueError(f"DPMSolverSampler: order={order!r}, the multistep solver is built for order 1 and 2")
        if skip_type not in schedules.DPM_SKIP_TYPES:
            raise ValueError(f"DPMSolverSampler: unknown skip_type {skip_type!r}, one of {schedules.DPM_SKIP_TYPES}")
        ac = self.model.alphas_cumprod.detach().double().cpu().numpy()
        self.timesteps, _ = schedules.dpm_solver_table(ac, S, skip_type, order, lower_order_final)      # a grid with no step: ValueError
        mode = self._check_guidance(conditioning, unconditional_conditioning, unconditional_guidance_scale, batch_size)
        if unconditional_guidance_scale != 1.:
            assert unconditional_conditioning is not None
        if verbose:
            print(f"Data shape for DPM-Solver++ sampling is {(batch_size, *shape)}, order {order}, {skip_type} grid of {len(self.timesteps)} steps")
        self.num_stage = num_stage
        solver = (int(order), skip_type, bool(lower_order_final))
        conds, composed, guide = _composed_call(comp, conditioning)

        def go(noise_src):
            eng = self._engine(batch_size, tuple(shape), mode, S, 0.0, unconditional_guidance_scale, num_stage, 1.0, replica, solver=solver,
                               composed=composed)
            return eng.run(conds, unconditional_conditioning, x_T=x_T, noise=noise_src, seed=seed, sample0=sample0,
                           log_every_t=log_every_t, callback=callback, img_callback=img_callback, model=self.model, **guide)
        from . import autoplanes
        return autoplanes.run(self.model.model.diffusion_model, go, f"{type(self).__name__}.sample", noise=noise)
