"""The diffusion objective on the HIP engine: FridoDiffusion.forward / p_losses of the reference (frido/models/diffusion/frido.py:1007-1050,
1180-1224) without a backward pass -- what its `test_step` / `validation_step` evaluate.

  LossEngine   -- per (B, H, W, context length, precision): for every stage  frido_qsample -> plan.pre -> plan.step -> frido_diffusion_loss,
                  the whole call captured once as a hipGraph.  Timesteps, seed, shard offset, the schedule tables and logvar are device
                  state, so another batch with other timesteps replays the same graph; results are device tensors.  With Philox noise and
                  device tensors for t, the tables and logvar nothing in a call makes the host wait for the stream; a host t, a host
                  noise tape or a changed host logvar is uploaded from pageable memory, and such an upload does make the host wait.

`plan.pre` runs on every call: the timestep table and the cross-attention K / V^T depend on the batch, and SPADE reads the noisy coarse
channels of this call's x_noisy.
"""
import collections
import ctypes as C

import torch

from . import _lib
from .builder import Builder
from .engine import Prog, lru_entry, own_stream
from .runtime import _relayout
from .unet_plan import UNetStagePlan

LOSS_TYPES = {"l1": 0, "l2": 1}


def launch_qsample(desc, stream):
    _lib.check(_lib.lib().frido_qsample(C.byref(desc), stream), "frido_qsample")


def launch_loss(desc, stream):
    _lib.check(_lib.lib().frido_diffusion_loss(C.byref(desc), stream), "frido_diffusion_loss")


class LossEngine:
    """The plans, the state and the results of one (B, H, W, context length, precision).  What the plans do not depend on is given per
    call: the schedule tables and logvar are copied into device state, the objective's scalars (loss type, noise_mix_ratio, the two
    weights) are descriptor fields of the two ops and the stages to run select the launches -- so they key the captured graphs
    (a handful of launches to record again), not the engine (two whole stage plans)."""
    GRAPHS = 8      # captured graphs kept per engine, least recently used first out

    def __init__(self, builder: Builder, cfg, **kw):
        self.planes = builder.planes
        with _lib.use_planes(self.planes):
            self._init(builder, cfg, **kw)

    def _init(self, builder, cfg, *, B, C, H, W, nctx, embed_dim, num_stage, T, use_graph=True):
        if not cfg.get("use_split_head", False):
            raise NotImplementedError("use_split_head=False: the objective compares the stage's own eps channels, which needs the split head "
                                      "(every shipped Frido config)")
        self.b, self.cfg, self.dev = builder, cfg, builder.device
        self.B, self.C, self.H, self.W, self.nctx = B, C, H, W, nctx
        self.embed, self.num_stage, self.use_graph = list(embed_dim), num_stage, use_graph
        assert sum(self.embed[:num_stage]) <= C, f"{num_stage} stages need a latent of {sum(self.embed[:num_stage])} channels, got {C}"
        dev, HW, S = self.dev, H * W, num_stage
        self.T = int(T)
        self.sqrt_ac, self.sqrt_1mac, self.lvlb, self.logvar = (torch.zeros(self.T, dtype=torch.float32, device=dev) for _ in range(4))
        self.labels = cfg.get("num_classes") is not None
        self.x0 = torch.zeros(B, HW, C, dtype=torch.float32, device=dev)
        self.t = torch.zeros(B, dtype=torch.int64, device=dev)
        self.rng = torch.zeros(2, dtype=torch.int64, device=dev)        # {seed, sample0} read by the captured kernels
        self.rows = torch.zeros(S, 4, dtype=torch.float32, device=dev)
        self.per_sample = torch.zeros(S, B, dtype=torch.float32, device=dev)
        self.tape = None                                                # [S][B][HW][C], allocated by the first host-noise call
        self.stages, self.x_noisy = [], []
        with self.b.persist_scope() as owned:                           # the engine owns its plans' persistent buffers
            for s in range(S):
                xn = torch.zeros(B, HW, sum(self.embed[:s + 1]), dtype=torch.float32, device=dev)
                self.x_noisy.append(xn)
                self.stages.append(UNetStagePlan(self.b, cfg, B=B, H=H, W=W, nctx=nctx, stage=s, x_state=xn, temb_rows=B, per_sample_t=True))
        self._persist = owned
        self.graphs = collections.OrderedDict()      # (tape?, stages, scalars) -> captured graph (or the program, use_graph=False)
        self.graph_captures = 0
        self._stream = None
        self._rng_host = (0, 0)
        self._logvar_zero = torch.zeros(self.T)
        self._logvar_host = self._logvar_zero

    def _set_logvar(self, logvar):
        """The device copy of the model's logvar.  A host tensor (the reference keeps it on the CPU unless it is learned) is uploaded only
        when its values changed: an upload from pageable memory makes the host wait for the stream, i.e. for the previous call's graph."""
        if logvar is None:
            logvar = self._logvar_zero
        logvar = logvar.detach().reshape(self.T)
        if logvar.is_cuda:
            self.logvar.copy_(logvar)
            self._logvar_host = None
        elif self._logvar_host is None or not torch.equal(self._logvar_host, logvar):
            self._logvar_host = logvar.to(torch.float32).clone()
            self.logvar.copy_(self._logvar_host)

    # ---- the launch sequence -------------------------------------------------------------------------------------------------------
    def _descs(self, s, tape, sc):
        """(FridoQSample, FridoDiffusionLoss) of stage s; tape: read the noise from self.tape[s], else Philox keyed (rng, stage);
        sc: (loss type number, mix_tau, l_simple_weight, original_elbo_weight)."""
        B, HW = self.B, self.H * self.W
        loss_type, mix_tau, lsw, elbo = sc
        start, nch = sum(self.embed[:s]), self.embed[s]
        noise = self.tape[s].data_ptr() if tape else None
        rng = None if tape else self.rng.data_ptr()
        q = _lib.STRUCTS["FridoQSample"](x0=self.x0.data_ptr(), x_noisy=self.x_noisy[s].data_ptr(), t=self.t.data_ptr(),
                                         sqrt_ac=self.sqrt_ac.data_ptr(), sqrt_1mac=self.sqrt_1mac.data_ptr(), noise=noise, rng_dev=rng,
                                         mix_tau=mix_tau, B=B, HW=HW, Cx=self.C, ch_start=start, ch_end=start + nch, T=self.T, rng_stream=s)
        plan = self.stages[s]
        assert plan.nch == nch
        ls = _lib.STRUCTS["FridoDiffusionLoss"](pred=plan.eps.data_ptr(), t=self.t.data_ptr(), noise=noise, rng_dev=rng,
                                                logvar=self.logvar.data_ptr(), lvlb_weights=self.lvlb.data_ptr(),
                                                per_sample=self.per_sample[s].data_ptr(), out=self.rows[s].data_ptr(), B=B, HW=HW, Cx=self.C,
                                                ch_start=start, nch=nch, T=self.T, rng_stream=s, loss_type=loss_type,
                                                l_simple_weight=lsw, original_elbo_weight=elbo)
        return q, ls

    def program(self, tape, stages, sc):
        """The whole call as one program: per stage of `stages` q_sample, the plan's two programs, the loss."""
        prog = Prog(self.dev, self.b.nsplit)
        for s in stages:
            plan = self.stages[s]
            q, ls = self._descs(s, tape, sc)
            prog.ops += ([_lib.op_of("FRIDO_OP_QSAMPLE", q)] + list(plan.pre.ops) + list(plan.step.ops)
                         + [_lib.op_of("FRIDO_OP_DIFFUSION_LOSS", ls)])
        prog.keep = list(self.stages)
        return prog

    # ---- main entry ----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    @_lib.with_planes
    def run(self, x, cond, t, *, tables, tape=None, seed=0, sample0=0, logvar=None, stages=None, loss_type="l1", mix_tau=0.,
            l_simple_weight=1., original_elbo_weight=0.):
        """x (B, C, H, W) f32 NCHW on the GPU, cond: the context (B, nctx, cd), class labels or None, t (B,) int64 (any device),
        tables: (sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, lvlb_weights), [T] tensors copied on every call (the model's
        buffers: device to device), so a schedule that changed is never served from an older copy,
        tape: None (Philox keyed by (seed, sample0 + b, stage)) or a list of num_stage host / device noise tensors (B, C, H, W), read
        for the stages that run, logvar: [T] tensor or None (zeros), stages: the stages to run (default: all).
        Returns (rows [S][4] = {loss_simple, loss_gamma, loss_vlb, loss} per stage, per-sample loss_simple [S][B]), device tensors
        of this call's own; the rows of a stage that did not run are whatever an earlier call left."""
        B, Cn, H, W = self.B, self.C, self.H, self.W
        assert tuple(x.shape) == (B, Cn, H, W), (tuple(x.shape), (B, Cn, H, W))
        if loss_type not in LOSS_TYPES:
            raise NotImplementedError(f"unknown loss type '{loss_type}'")
        stages = tuple(range(self.num_stage)) if stages is None else tuple(int(s) for s in stages)
        assert stages and all(0 <= s < self.num_stage for s in stages), stages
        sc = (LOSS_TYPES[loss_type], float(mix_tau), float(l_simple_weight), float(original_elbo_weight))
        with own_stream(self, self.dev) as sp:
            _relayout(self.b, sp, x.contiguous().float(), self.x0, B, H * W, Cn, 0)
            self.t.copy_(torch.as_tensor(t, dtype=torch.int64).reshape(B))
            for dst, src in zip((self.sqrt_ac, self.sqrt_1mac, self.lvlb), tables):
                dst.copy_(torch.as_tensor(src).detach().reshape(self.T))
            self._set_logvar(logvar)
            for plan in (self.stages[s] for s in stages):
                plan.set_timesteps(self.t)
                if self.labels:
                    plan.set_labels(cond)
                elif cond is not None and plan.ctx_in is not None:
                    plan.set_context(cond.to(self.dev, torch.float32))
            if tape is not None:
                assert len(tape) == self.num_stage
                if self.tape is None:
                    self.tape = torch.empty(self.num_stage, B, H * W, Cn, dtype=torch.float32, device=self.dev)
                for s in stages:                                          # plumbing: layout + H2D
                    n = tape[s]
                    self.tape[s].copy_(torch.as_tensor(n, dtype=torch.float32).reshape(B, Cn, H * W).permute(0, 2, 1))
            elif self._rng_host != (int(seed), int(sample0)):
                self._rng_host = (int(seed), int(sample0))
                self.rng[0].fill_(self._rng_host[0])                      # scalar kernel arguments: no host buffer the stream would wait for
                self.rng[1].fill_(self._rng_host[1])
            key = ("tape" if tape is not None else "philox", stages, sc)

            def capture():
                prog = self.program(tape is not None, stages, sc)
                g = prog.capture(sp) if self.use_graph else prog
                self.graph_captures += 1
                return g
            # (rare) a graph must not go while a replay of it is queued: the stream is drained before one is dropped
            g = lru_entry(self.graphs, key, self.GRAPHS, capture, before_evict=self._stream.synchronize)
            g.launch(sp) if self.use_graph else g.run(sp)
            return self.rows.clone(), self.per_sample.clone()
