"""Compiles the Frido denoiser (reference: frido/modules/diffusionmodules/pyunet.py:867-950) into
HIP programs for one (batch, latent size, context length, stage).

Two programs per stage:
  * pre  — everything that does not change from step to step and is hoisted out of the sampling loop
           (SURVEY.md §0 facts 8, §2b K9/K10): the timestep/stage embedding table for all S steps and
           the per-ResBlock `emb_layers` projections of it, cross-attention K / V^T of the context,
           and (stage >= 1) the SPADE conditioning feature map with every gamma/beta map;
  * step — one denoiser forward reading the NHWC f32 latent state and writing eps.
Layout: activations NHWC, f32 residual stream + bf16 (hi/lo) operand tensors feeding the MFMA GEMM.
"""
import numpy as np
import torch

from .arch import unet_arch
from .builder import Builder, ACT_NONE, ACT_RELU, ACT_SILU
from .engine import pack_matrix, rup

import os
# ERROR-BUDGET EXPERIMENTS (tools/x3_single_plane_table.py, profiles/r03_x3_single_plane_table.txt): keep ONE bf16 plane of an operand
# class inside the bf16x3 mode.  Off by default -- every one of them fails the parity bar.
X3_SPADE_BF16 = os.environ.get("FRIDO_X3_SPADE_BF16", "0") != "0"       # hoisted SPADE gamma / beta maps stored as bf16
X3_CROSSKV_HI = os.environ.get("FRIDO_X3_CROSSKV_HI", "0") != "0"       # cached cross-attention K / V^T: residual (lo) planes zeroed


class _Shape:
    """Stand-in for an activation that does not exist yet (only its channel count matters to Builder.gn_conv_tile)."""

    def __init__(self, C):
        self.C, self.bf16 = C, False


class UNetStagePlan:
    def __init__(self, b: Builder, cfg, *, B, H, W, nctx, stage, x_state, temb_rows, per_sample_t, step_ptr=None,
                 xrep=1, step_bx_ptr=None):
        """x_state: f32 device tensor [B][H*W][Ctot] (NHWC latent).  The denoiser runs on a logical batch
        Bx = B * xrep (xrep = 2 for classifier-free guidance: [cond | uncond] share x, differ in context).
        temb_rows: number of rows of the timestep table (S in sampler mode, Bx when per_sample_t).
        step_bx_ptr (class-conditional denoisers in sampler mode): a second device counter that advances by Bx per step -- the
        embedding table then has one row per (step, sample), S * Bx in all, and a ResBlock row m reads row m / HW + *step_bx."""
        self.b, self.cfg = b, cfg
        a = self.a = unet_arch(cfg)
        self.B, self.H, self.W, self.nctx, self.stage, self.xrep = B, H, W, nctx, stage, xrep
        self.Bx = B * xrep
        self.x_state = x_state
        self.Ctot = x_state.shape[-1]
        self.per_sample_t = per_sample_t
        self.step_ptr = step_ptr
        self.step_bx_ptr = step_bx_ptr
        self.table_per_sample = a.num_classes is not None and not per_sample_t
        assert not self.table_per_sample or step_bx_ptr, "a class-conditional sampler plan needs the per-sample step counter"
        self.temb_rows = temb_rows
        dev = b.device
        self.t_dev = torch.zeros(temb_rows, dtype=torch.int64, device=dev)
        # cross-attention context: SpatialTransformer denoisers only (the AttentionBlock family has none, pyunet.py:513-517)
        self.ctx_in = torch.zeros(self.Bx, nctx, a.context_dim, dtype=torch.float32, device=dev) if a.context_dim is not None else None
        # class labels (pyunet.py:885-888): one per logical sample -- int64 indices (nn.Embedding) or float rows (nn.Linear)
        self.y_in = None
        if a.num_classes is not None:
            self.y_in = (torch.zeros(self.Bx, dtype=torch.int64, device=dev) if a.use_embed
                         else torch.zeros(self.Bx, a.num_classes, dtype=torch.float32, device=dev))
        self.nch = a.splits[stage] if a.use_split_head else cfg["out_channels"]
        self.eps = torch.zeros(self.Bx * H * W, self.nch, dtype=torch.float32, device=dev)
        self.c0 = sum(a.splits[:stage]) if (a.use_split_head and a.use_spade) else 0
        self.c1 = sum(a.splits[:stage + 1]) if a.use_split_head else a.in_channels
        self.spade_on = a.use_spade and self.c0 > 0
        # names of every ResBlock in forward order (for the concatenated emb_layers projection)
        self.res_names = [blk.prefix for grp in (a.input_blocks + [a.middle] + a.output_blocks) for blk in grp
                          if blk.kind == "res"]
        self.res_cout = [blk.cout for grp in (a.input_blocks + [a.middle] + a.output_blocks) for blk in grp
                         if blk.kind == "res"]
        self.res_off = np.concatenate([[0], np.cumsum(self.res_cout)]).astype(int)
        self.E = b.persistent_f32(temb_rows * (self.Bx if self.table_per_sample else 1), int(self.res_off[-1]))
        self.kv = {}        # ST prefix -> (k operand [Bx*nctx][C], vT operand [Bx][C][nctx_pad])
        self.spade = {}     # SPADE module prefix -> (gamma F32-like, beta)
        self.pre = self._build_pre()
        self.step = self._build_step()

    # ------------------------------------------------------------------------------------------
    class _T:  # persistent f32 tensor wrapper with the F32 interface
        def __init__(self, t):
            self.t = t
            self.rows, self.C = t.shape[0], t.shape[1]

        @property
        def ptr(self):
            return self.t.data_ptr()

        def free(self):
            pass

    def _persistent_act(self, rows, C):
        """Persistent [rows][C] activation in the stream dtype (bf16 in bf16 mode, f32 in bf16x3 mode)."""
        b = self.b
        as_bf16 = b.stream_bf16 or X3_SPADE_BF16
        t = torch.empty(rows, C, dtype=torch.bfloat16 if as_bf16 else torch.float32, device=b.device)
        b._persist.append(t)
        w = self._T(t)
        w.bf16 = as_bf16
        return w

    def _pack_x(self, c0, c1):
        """operand [Bx*HW][32] of latent channels [c0, c1) (replicated xrep times)."""
        b, HW = self.b, self.H * self.W
        o = b.op(self.Bx * HW, rup(c1 - c0, 32))
        for r in range(self.xrep):
            b.prog.emit("FRIDO_OP_PACK", src=self.x_state.data_ptr(), B=self.B, HW=HW, Csrc=self.Ctot, c0=c0,
                        Cuse=c1 - c0, Cpad=o.K, nchw=0, scale=1.0, nsplit=b.nsplit,
                        out_op=o.ptr + 2 * r * self.B * HW * o.K, out_lo=o.lo)
        return o

    def _build_pre(self):
        b, a = self.b, self.a
        prog = b.new_prog()
        mc, te = a.model_channels, a.time_embed_dim
        # ---- timestep / stage embedding table (util.py:151-171, pyunet.py:560-565,882-896) ----
        n = self.temb_rows
        sin = b.f32_strict(n, mc)
        prog.emit("FRIDO_OP_TIME_EMB", t=self.t_dev.data_ptr(), n=n, dim=mc, max_period=10000.0, out=sin.ptr)
        sin_op = b.pack(sin.ptr, 1, n, mc, 0, mc)
        sin.free()
        h1 = b.linear(sin_op, "time_embed.0", act=ACT_SILU, out="op")
        sin_op.free()
        bias2 = b.w["time_embed.2.bias"].float()
        if a.num_stage > 1:
            bias2 = bias2 + b.w["stage_emb.weight"][self.stage].float()
        bias2 = bias2.contiguous()
        b._persist.append(bias2)
        if a.num_classes is None:
            semb = b.linear(h1, "time_embed.2", bias_ptr=bias2.data_ptr(), act=ACT_SILU, out="op")   # SiLU(emb)
        else:
            semb = self._label_semb(h1, bias2, n)
        h1.free()
        wcat = b.cat_lin_weight("emb_cat", [f"{p}.emb_layers.1.weight" for p in self.res_names])
        bcat = torch.cat([b.w[f"{p}.emb_layers.1.bias"].float() for p in self.res_names]).contiguous()
        b._persist.append(bcat)
        b.linear(semb, None, wop=wcat, bias_ptr=bcat.data_ptr(), out=("f32", self._T(self.E)))
        semb.free()
        # ---- cross-attention K / V^T of the context (attention.py:175-176), once per sample ----
        ctx_op = b.pack(self.ctx_in.data_ptr(), 1, self.Bx * self.nctx, a.context_dim, 0, a.context_dim) if self.ctx_in is not None else None
        for grp in a.input_blocks + [a.middle] + a.output_blocks:
            for blk in grp:
                if blk.kind != "st" or ctx_op is None:
                    continue
                for dpt in range(a.transformer_depth):
                    t = f"{blk.prefix}.transformer_blocks.{dpt}.attn2"
                    C = blk.cin
                    k = b.persistent_op(self.Bx * self.nctx, C, zero=False)
                    wkq, _ = b.folded_qk_weight(t + ".to_q", t + ".to_k", "k")
                    b.linear(ctx_op, None, wop=wkq, bias=False, out=("op", k))
                    wvo, bvo = b.folded_vo_weight(t + ".to_v", t + ".to_out.0")
                    vT = b.v_transposed(ctx_op, a.context_dim, wvo, self.Bx, self.nctx, C)
                    if X3_CROSSKV_HI and b.nsplit == 2:
                        for o_ in (k, vT):      # zero the residual planes: the cache then carries 8 mantissa bits
                            prog.emit("FRIDO_OP_FILL", dst=o_.ptr + 2 * o_.lo, n=o_.lo // 2, value=0)
                    self.kv[(blk.prefix, dpt)] = (k, vT, bvo)
        if ctx_op is not None:
            ctx_op.free()
        # ---- SPADE conditioning (spade_norm.py:44-60), timestep-invariant within a stage ----
        if self.spade_on:
            HW = self.H * self.W
            xc = self._pack_x(0, self.c0)
            hc = b.conv(xc, self.Bx, self.H, self.W, f"pre_input_cond_blocks.{self.stage - 1}.0", out="op")
            xc.free()
            for name, C, lvl in self._spade_sites():
                Hl, Wl = self.H >> lvl, self.W >> lvl
                actv = b.conv(hc, self.Bx, self.H, self.W, name + ".mlp_shared.0", dn=lvl, act=ACT_RELU, out="op")
                g = self._persistent_act(self.Bx * Hl * Wl, C)
                be = self._persistent_act(self.Bx * Hl * Wl, C)
                b.conv(actv, self.Bx, Hl, Wl, name + ".mlp_gamma", out=("f32", g))
                b.conv(actv, self.Bx, Hl, Wl, name + ".mlp_beta", out=("f32", be))
                actv.free()
                self.spade[name] = (g, be)
            hc.free()
        return prog

    def _spade_sites(self):
        """(SPADE module prefix, channels, resolution level) for every SPADE instance in forward order."""
        a = self.a
        out, lvl = [], 0
        for grp in a.input_blocks:
            for blk in grp:
                if blk.kind == "res":
                    out += [(blk.prefix + ".in_layers.0", blk.cin, lvl), (blk.prefix + ".out_layers.0", blk.cout, lvl)]
                elif blk.kind in ("st", "attn"):
                    out.append((blk.prefix + ".norm", blk.cin, lvl))
                elif blk.kind == "down":
                    lvl += 1
        for blk in a.middle:
            if blk.kind == "res":
                out += [(blk.prefix + ".in_layers.0", blk.cin, lvl), (blk.prefix + ".out_layers.0", blk.cout, lvl)]
            else:
                out.append((blk.prefix + ".norm", blk.cin, lvl))
        for grp in a.output_blocks:
            for blk in grp:
                if blk.kind == "res":
                    out += [(blk.prefix + ".in_layers.0", blk.cin, lvl), (blk.prefix + ".out_layers.0", blk.cout, lvl)]
                elif blk.kind in ("st", "attn"):
                    out.append((blk.prefix + ".norm", blk.cin, lvl))
                elif blk.kind == "up":
                    lvl -= 1
        return out

    # ------------------------------------------------------------------------------------------
    def _norm(self, x1, x2, HW, name, eps, act, want_raw=False, x1_dead=False):
        """GroupNorm32 / Normalize, SPADE-wrapped when the config says so (pyunet.py:209,233; attention.py:260)."""
        b = self.b
        if self.a.use_spade:
            g, be = self.spade.get(name, (None, None))
            return b.groupnorm(x1, x2, self.Bx, HW, name + ".param_free_norm", eps, gamma=g, beta=be, act=act,
                               want_raw=want_raw, x1_dead=x1_dead)
        return b.groupnorm(x1, x2, self.Bx, HW, name, eps, act=act, want_raw=want_raw, x1_dead=x1_dead)

    def _rowvec(self, ridx):
        d = dict(ptr=self.E.data_ptr() + 4 * int(self.res_off[ridx]), ld=int(self.res_off[-1]))
        if self.per_sample_t:
            d["rows_per_vec"] = None     # filled by caller (HW at that resolution)
        elif self.table_per_sample:
            d["rows_per_vec"] = None     # row (step, sample) = m / HW + step * Bx
            d["step"] = self.step_bx_ptr
        else:
            d["rows_per_vec"] = 1 << 30  # every row uses the row selected by the step counter
            d["step"] = self.step_ptr
        return d

    def _norm_params(self, name):
        """(parameter prefix, gamma, beta) of a GroupNorm32 / SPADE site (pyunet.py:209,233; spade_norm.py:44-60)."""
        if self.a.use_spade:
            g, be = self.spade.get(name, (None, None))
            return name + ".param_free_norm", g, be
        return name, None, None

    def _res_block(self, blk, x1, x2, h, w, ridx):
        """pyunet.py:262-300.  x1 (+x2 = skip tensor, virtual concat).  Returns F32 [Bx*h*w][cout]."""
        b, HW = self.b, h * w
        pre = blk.prefix
        has_skip = (pre + ".skip_connection.weight") in b.w
        rv = self._rowvec(ridx)
        if rv["rows_per_vec"] is None:
            rv["rows_per_vec"] = HW
        # r04: on the 64^2 / 32^2 planes both GroupNorm-apply passes ride inside the convs that consume them (csrc/convgn.inc)
        n1, g1, be1 = self._norm_params(pre + ".in_layers.0")
        n2, g2, be2 = self._norm_params(pre + ".out_layers.0")
        bf16_maps = any(getattr(m, "bf16", False) for m in (g1, g2) if m is not None)
        t1 = 0 if bf16_maps else b.gn_conv_tile(x1, x2, self.Bx, h, w, blk.cout)
        if t1 and has_skip:
            Craw = x1.C + (x2.C if x2 is not None else 0)
            if Craw % 64:
                t1 = 0
        t2 = b.gn_conv_tile(_Shape(blk.cout), None, self.Bx, h, w, blk.cout, raw=(x1, x2) if has_skip else None) if t1 else 0
        if t1 and t2:
            hmid = b.gn_conv(t1, x1, x2, self.Bx, h, w, n1, 1e-5, pre + ".in_layers.2", gamma=g1, beta=be1, rowvec=rv)
            if has_skip:
                out = b.gn_conv(t2, hmid, None, self.Bx, h, w, n2, 1e-5, pre + ".out_layers.3", gamma=g2, beta=be2,
                                skip=(x1, x2, pre + ".skip_connection"))
            else:
                assert x2 is None
                out = b.gn_conv(t2, hmid, None, self.Bx, h, w, n2, 1e-5, pre + ".out_layers.3", gamma=g2, beta=be2, residual=x1)
            hmid.free()
            return out
        a1, raw = self._norm(x1, x2, HW, pre + ".in_layers.0", 1e-5, ACT_SILU, want_raw=has_skip)
        hmid = b.conv(a1, self.Bx, h, w, pre + ".in_layers.2", rowvec=rv)
        a1.free()
        a2, _ = self._norm(hmid, None, HW, pre + ".out_layers.0", 1e-5, ACT_SILU, x1_dead=True)     # hmid feeds this norm only
        hmid.free()
        if has_skip and raw.K % 64 == 0 and a2.K % 64 == 0:
            out = b.conv_plus_skip(a2, raw, self.Bx, h, w, pre + ".out_layers.3", pre + ".skip_connection")
            raw.free()
        elif has_skip:
            res = b.linear(raw, pre + ".skip_connection")
            raw.free()
            out = b.conv(a2, self.Bx, h, w, pre + ".out_layers.3", residual=res, out=("f32", res))
        else:
            assert x2 is None
            out = b.conv(a2, self.Bx, h, w, pre + ".out_layers.3", residual=x1)
        a2.free()
        return out

    def _spatial_transformer(self, blk, x, h, w):
        """attention.py:289-326 with BasicTransformerBlock._forward (222-227), single head d = C."""
        b, HW, C, Bx = self.b, h * w, blk.cin, self.Bx
        pre = blk.prefix
        a0, _ = self._norm(x, None, HW, pre + ".norm", 1e-6, ACT_NONE)
        hcur = b.linear(a0, pre + ".proj_in")
        a0.free()
        depth = self.a.transformer_depth
        for dpt in range(depth):        # attention.py:274-277,321-322 (every shipped config: depth 1)
            hcur = self._transformer_block(pre, dpt, hcur, x if dpt == depth - 1 else None, HW, C)     # (frees its input stream)
        return hcur

    def _transformer_block(self, pre, dpt, hcur, x, HW, C):
        """BasicTransformerBlock._forward (attention.py:222-227).  `x` is the SpatialTransformer's input for the LAST block
        (its feed-forward is then chained with proj_out + x into one GEMM), None for the inner blocks of a deeper transformer,
        which return the token stream itself."""
        b, Bx = self.b, self.Bx
        last = x is not None
        t = f"{pre}.transformer_blocks.{dpt}"
        # --- self-attention
        n1 = b.layernorm(hcur, t + ".norm1")
        # scores: q' = n1 (W_q^T W_k) against the raw rows of n1 (the key projection is folded into the query side)
        wq, _ = b.folded_qk_weight(t + ".attn1.to_q", t + ".attn1.to_k", "q")
        Np = rup(HW, 32)
        if (C, HW) not in self._vt_self:
            self._vt_self[(C, HW)] = b.persistent_op(C, Np, batch=Bx, zero=True)
        vT = self._vt_self[(C, HW)]
        # the single-head output projection is folded into V: PV lands directly on the residual stream
        wvo, bvo = b.folded_vo_weight(t + ".attn1.to_v", t + ".attn1.to_out.0")
        with b.gemm_pair():      # two projections of the same rows, independent of each other
            b.v_transposed(n1, C, wvo, Bx, HW, C, out=vT)
            qp = b.linear(n1, None, wop=wq, bias=False, out="op")
        kc, vTc, bvo2 = self.kv[(pre, dpt)]     # kc = ctx (W_q^T W_k)^T: the query projection is folded into the cached keys
        chain = last and C % 64 == 0       # proj_out(h3 + ff2(gg)) + x in ONE GEMM (needs h3 as an operand along K)
        if b.attention_chain_ok(C, C, HW, C, self.nctx, C):
            # the 32 x 32 plane: the flash launch owns whole rows of h2 / n2 and runs the 26-key cross-attention and norm3 on them
            # itself -- one launch, and neither tensor makes the round trip through HBM (csrc/flash.hip, the cross tail)
            h3 = b.attention_chain(qp, C, n1, C, vT, Bx, HW, HW, C, bias_ptr=bvo, residual=hcur, ln=(t + ".norm2", 1e-5), k2=kc, ldk2=C,
                                   vT2=vTc, Nk2=self.nctx, bias2_ptr=bvo2, ln2=(t + ".norm3", 1e-5), also_op=chain, stream_dead=chain)
            qp.free()
            n1.free()
            hcur.free()
        else:
            h2 = b.attention(qp, C, n1, C, vT, Bx, HW, HW, C, bias_ptr=bvo, residual=hcur, stream=True, ln=(t + ".norm2", 1e-5))
            qp.free()
            n1.free()
            hcur.free()
            # --- cross-attention (K, V^T cached per sample)
            n2 = getattr(h2, "ln_copy", None)       # (r03) the attention kernel's epilogue may have produced it
            if n2 is None:
                n2 = b.layernorm(h2, t + ".norm2")
            # (r05) with FF2 + proj_out chained, h3 is read only as an operand (A2 of that GEMM) and through norm3: where the kernel
            # produces both copies itself the f32 rows are not stored at all
            h3 = b.attention(n2, C, kc, C, vTc, Bx, HW, self.nctx, C, bias_ptr=bvo2, residual=h2, stream=True, also_op=chain,
                             ln=(t + ".norm3", 1e-5), stream_dead=chain)
            n2.free()
            h2.free()
        # --- GEGLU feed-forward (attention.py:37-64)
        n3 = getattr(h3, "ln_copy", None)
        if n3 is None:
            n3 = b.layernorm(h3, t + ".norm3")
        gg = b.linear_geglu(n3, t + ".ff.net.0.proj")
        n3.free()
        if not last:
            out = b.linear(gg, t + ".ff.net.2", residual=h3)     # the next block's token stream
            gg.free()
            h3.free()
            return out
        h3op = h3 if b.stream_bf16 else getattr(h3, "op_copy", None)     # bf16 stream: the activation is its own operand
        if chain and h3op is not None:
            # ff2 and proj_out are both linear: [gg | h3] . [W_p W_f | W_p]^T + (W_p b_f + b_p) + x (weights folded in float64);
            # in bf16x3 mode h3's operand copy comes from the cross-attention kernel's epilogue (r03: one launch and the h4
            # round trip less per transformer block)
            out = b.chained_linear(gg, h3op, t + ".ff.net.2", pre + ".proj_out", x)
            gg.free()
            if h3op is not h3:
                h3op.free()
            h3.free()
            return out
        assert not getattr(h3, "stream_skipped", False)      # the unchained tail reads h3's f32 rows
        h4 = b.linear(gg, t + ".ff.net.2", residual=h3, out="op")
        gg.free()
        h3.free()
        out = b.linear(h4, pre + ".proj_out", residual=x)
        h4.free()
        return out

    def _attention_block(self, blk, x, h, w):
        """AttentionBlock._forward (pyunet.py:346-358): norm -> qkv (1x1) -> QKVAttention[Legacy] over blk.heads heads -> proj_out + x."""
        b, HW, C, Bx = self.b, h * w, blk.cin, self.Bx
        pre, heads = blk.prefix, blk.heads
        d = C // heads
        a0, _ = self._norm(x, None, HW, pre + ".norm", 1e-5, ACT_NONE)
        if (C, HW) not in self._vt_self:
            self._vt_self[(C, HW)] = b.persistent_op(C, rup(HW, 32), batch=Bx, zero=True)
        vT = self._vt_self[(C, HW)]
        # V rows of the qkv weight, head-major (head h = rows h d ..): 3 d h + 2 d + j after a heads-first split (QKVAttentionLegacy,
        # pyunet.py:399), 2 C + h d + j after a qkv-first split (QKVAttention, :431).  One head: 2 C .. in both.
        hh, jj = torch.arange(heads)[:, None], torch.arange(d)[None, :]
        vrows = ((2 * C + hh * d + jj) if (blk.new_order or heads == 1) else (3 * d * hh + 2 * d + jj)).flatten()
        key = ("attn_v", pre, heads == 1)
        if key not in b._wcache:
            wqkv, bqkv = b.h64(pre + ".qkv.weight"), b.h64(pre + ".qkv.bias")
            wv, bv = wqkv[vrows], bqkv[vrows]
            if heads == 1:      # W_o (P (X W_v^T + b_v)) + b_o = P (X (W_o W_v)^T) + (W_o b_v + b_o): the rows of P sum to one
                wo = b.h64(pre + ".proj_out.weight")
                wv, bv = wo @ wv, wo @ bv + b.h64(pre + ".proj_out.bias")
            b._wcache[key] = (pack_matrix(b.to_dev(wv), b.nsplit), b.to_dev(bv))
        wv_op, bv_dev = b._wcache[key]
        with b.gemm_pair():      # two projections of the same rows, independent of each other
            b.v_transposed(a0, C, wv_op, Bx, HW, C, bias_ptr=None if heads == 1 else bv_dev.data_ptr(), out=vT)
            if heads == 1:
                # one head, any width: q | k = the first 2 C rows of the projection, the existing single-head kernels, proj_out folded
                # into V so that P V + bias + x lands on the residual stream
                qk = b.linear(a0, None, wop=b.lin_weight(pre + ".qkv.weight", rows=(0, 2 * C)), bias_ptr=b.bias(pre + ".qkv.bias"), out="op")
            else:
                qkv = b.linear(a0, pre + ".qkv", out="op")            # [Bx*HW][3 C]: q and k stay where the projection left them
        if heads == 1:
            out = b.attention(qk, 2 * C, qk, 2 * C, vT, Bx, HW, HW, C, q_off=0, k_off=C, bias_ptr=bv_dev.data_ptr(), residual=x, stream=True)
            qk.free()
            a0.free()
            return out
        o = b.attention_heads(qkv, 3 * C, vT, Bx, HW, heads, d, legacy=not blk.new_order)
        qkv.free()
        a0.free()
        out = b.linear(o, pre + ".proj_out", residual=x)
        o.free()
        return out

    def _label_semb(self, h1, bias2, n):
        """SiLU(time_embed(t_emb) + label_emb(y) [+ stage_emb]) as an operand (pyunet.py:883-896 + the SiLU of every emb_layers).
        The label embedding L [Bx][te] is computed first (a row gather for nn.Embedding, a small GEMM for nn.Linear) and enters the
        time_embed.2 GEMM as its row vector -- inside the activation, where the reference adds it.
        Forward mode (n == Bx rows, one timestep per sample): row m takes L[m].
        Sampler mode (n == S rows, one per step): the table gets S * Bx rows, row i * Bx + z = (step i, sample z): one S-row GEMM per
        sample z with L[z] as a launch-wide vector, written with a row stride of Bx rows."""
        b, a, Bx = self.b, self.a, self.Bx
        te = a.time_embed_dim
        if a.use_embed:
            L = b.f32_strict(Bx, te)
            b.prog.emit("FRIDO_OP_EMBED", tokens=self.y_in.data_ptr(), tok=b.dev_f32("label_emb.weight").data_ptr(), pos=None, out=L.ptr,
                        rows=Bx, n=Bx, D=te, vocab=a.num_classes)
        else:
            y_op = b.pack(self.y_in.data_ptr(), 1, Bx, a.num_classes, 0, a.num_classes)
            L = b.linear(y_op, "label_emb", out="f32_strict")
            y_op.free()
        wop = b.lin_weight("time_embed.2.weight")
        if self.per_sample_t:
            semb = b.linear(h1, "time_embed.2", bias_ptr=bias2.data_ptr(), act=ACT_SILU, out="op",
                            rowvec=dict(ptr=L.ptr, rows_per_vec=1, ld=te))
        else:
            semb = b.op(n * Bx, te)
            for z in range(Bx):
                b.prog.gemm(n, te, wop.K, h1, wop, bias=bias2.data_ptr(), rowvec=L.ptr + 4 * z * te, rows_per_vec=1 << 30, ldv=te,
                            act=ACT_SILU, out_op=semb.ptr + 2 * z * te, ldoo=Bx * te, oo_lo=semb.lo)
        L.free()
        return semb

    def _build_step(self):
        b, a = self.b, self.a
        prog = b.new_prog()
        self._vt_self = {}
        H, W = self.H, self.W
        s = self.stage
        xin = self._pack_x(self.c0, self.c1)
        head = f"pre_input_blocks.{s}.0" if a.use_split_head else "input_blocks.0.0"
        hcur = b.conv(xin, self.Bx, H, W, head)
        xin.free()
        hs = [(hcur, H, W)]
        h, w = H, W
        ridx = 0
        for grp in a.input_blocks:
            cur = hs[-1][0]
            first = True
            for blk in grp:
                if blk.kind == "res":
                    nxt = self._res_block(blk, cur, None, h, w, ridx)
                    ridx += 1
                elif blk.kind == "st":
                    nxt = self._spatial_transformer(blk, cur, h, w)
                elif blk.kind == "attn":
                    nxt = self._attention_block(blk, cur, h, w)
                elif blk.kind == "down":
                    xo = b.to_operand(cur)
                    nxt = b.conv(xo, self.Bx, h, w, blk.prefix + ".op", stride=2, pad=1)
                    xo.free()
                    h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
                if not first:
                    cur.free()      # intermediate inside the group (not a skip)
                cur, first = nxt, False
            hs.append((cur, h, w))
        cur = hs[-1][0]
        mid_in = cur
        for i, blk in enumerate(a.middle):
            if blk.kind == "res":
                nxt = self._res_block(blk, cur, None, h, w, ridx)
                ridx += 1
            elif blk.kind == "attn":
                nxt = self._attention_block(blk, cur, h, w)
            else:
                nxt = self._spatial_transformer(blk, cur, h, w)
            if cur is not mid_in:
                cur.free()
            cur = nxt
        for grp in a.output_blocks:
            skip, sh, sw = hs.pop()
            assert (sh, sw) == (h, w)
            first = True
            for blk in grp:
                if blk.kind == "res":
                    nxt = self._res_block(blk, cur, skip if first else None, h, w, ridx)
                    ridx += 1
                elif blk.kind == "st":
                    nxt = self._spatial_transformer(blk, cur, h, w)
                elif blk.kind == "attn":
                    nxt = self._attention_block(blk, cur, h, w)
                elif blk.kind == "up":
                    xo = b.to_operand(cur)
                    nxt = b.upsample_conv(xo, self.Bx, h, w, blk.prefix + ".conv")
                    xo.free()
                    h, w = h * 2, w * 2
                cur.free()
                if first:
                    skip.free()
                cur, first = nxt, False
        assert not hs
        o = f"out.{s}" if a.use_split_head else "out"
        eps_out = self._T(self.eps)
        if b.gn_conv_tiny_ok(cur, self.Bx, h, w, eps_out.C):
            # (r06) the eps head as ONE launch: GroupNorm statistics (from the producer's partial sums) + conv3x3_gn_tiny_kernel.  Until r05:
            # gn_apply (50 MB of operand planes written) + a 64-column MFMA tile for 3 live columns under split-K + its reduction
            b.gn_conv_tiny(cur, self.Bx, h, w, o + ".0", 1e-5, o + ".2", eps_out)
            cur.free()
            return prog
        ao, _ = b.groupnorm(cur, None, self.Bx, h * w, o + ".0", 1e-5, act=ACT_SILU)
        cur.free()
        b.conv(ao, self.Bx, h, w, o + ".2", out=("f32", eps_out))
        ao.free()
        return prog

    # ------------------------------------------------------------------------------------------
    def set_context(self, ctx):
        """ctx: device f32 [Bx][nctx][context_dim]."""
        self.ctx_in.copy_(ctx)

    def set_labels(self, y):
        """y: class labels of the Bx logical samples, int64 [Bx] (nn.Embedding) or float [Bx][num_classes] (nn.Linear)."""
        self.y_in.copy_(y.to(self.y_in.device, self.y_in.dtype))

    def set_timesteps(self, t):
        self.t_dev.copy_(t)
