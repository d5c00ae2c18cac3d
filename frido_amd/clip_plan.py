"""Compiles the text tower of OpenAI CLIP (the `encode_text` path FrozenCLIPTextEmbedder calls,
frido/modules/encoders/modules.py:188-219 -> clip/model.py `CLIP.encode_text`) into a HIP program:

    x = token_embedding[tokens] + positional_embedding                       (embed kernel)
    12 x ResidualAttentionBlock: x += out_proj(MHA_causal(ln_1(x)));  x += c_proj(QuickGELU(c_fc(ln_2(x))))
    z = ln_final(x)[b, argmax(tokens[b])] @ text_projection                  (row gather + GEMM)
    z = z / ||z||_2                                                          (l2norm kernel, `normalize=True`)

The attention is the (batch x head) QK^T GEMM -> causal row softmax -> PV GEMM chain the BERT plan uses; the causal mask is a
per-row key count inside the softmax kernel (FridoSoftmax.causal_nq).  The `clip` package is not a file of the reference
(it is a pip dependency, unpinned: environment.yaml `git+https://github.com/openai/CLIP.git@main`), so the algorithm is
restated from its published model.py; parity is pinned against oracle/clip_text.py only (no reference goldens exist).

ClipImagePlan (below) is the image tower, `encode_image`: the same blocks without the mask behind a patch-embedding GEMM, pinned
against the float64 restatement of tests/clip_vision_ref.py."""
import torch

from .builder import Builder
from .engine import rup

ACT_QUICKGELU = 4


def resblocks(b, prog, x, p, *, B, n, width, layers, heads, causal):
    """`layers` x clip/model.py ResidualAttentionBlock over the f32 rows x [B * n][width] (freed; the new stream is returned), weights
    under `p`transformer.resblocks.N: x += out_proj(MHA(ln_1(x)));  x += c_proj(QuickGELU(c_fc(ln_2(x)))).  causal: the text tower's
    mask (FridoSoftmax.causal_nq = n); the image tower attends everywhere.  Both towers emit exactly these ops."""
    H, dh = heads, width // heads
    Np = rup(n, 32)
    vT = b.persistent_op(width, Np, batch=B, zero=True)
    for layer in range(layers):
        r = f"{p}transformer.resblocks.{layer}"
        hn = b.layernorm(x, r + ".ln_1")
        inb = b.dev_f32(r + ".attn.in_proj_bias")
        wqk = b.lin_weight(r + ".attn.in_proj_weight", rows=(0, 2 * width))
        qk = b.op(B * n, 2 * width)
        b.linear(hn, None, wop=wqk, bias_ptr=inb.data_ptr(), out=("op", qk))
        wv = b.lin_weight(r + ".attn.in_proj_weight", rows=(2 * width, 3 * width))
        b.v_transposed(hn, width, wv, B, n, width, bias_ptr=inb.data_ptr() + 4 * 2 * width, out=vT)
        hn.free()
        s = b.f32_strict(B * H * n, n)
        prog.gemm(n, n, dh, qk, (qk.ptr + 2 * width, qk.lo), batch=B * H, batch_inner=H, lda=2 * width, ldb=2 * width,
                  a_bs=n * 2 * width, a_bs2=dh, b_bs=n * 2 * width, b_bs2=dh, alpha=float(dh) ** -0.5,
                  out_f32=s.ptr, of_bs=H * n * n, of_bs2=n * n, ldo=n)
        pr = b.softmax(s, B * H * n, n, n, Np, causal_nq=n if causal else 0)
        s.free()
        o = b.op(B * n, width)
        prog.gemm(n, dh, Np, pr, vT, batch=B * H, batch_inner=H, lda=Np, ldb=Np, a_bs=H * n * Np, a_bs2=n * Np,
                  b_bs=width * Np, b_bs2=dh * Np, out_op=o.ptr, oo_bs=n * width, oo_bs2=dh, ldoo=width, oo_lo=o.lo)
        pr.free()
        qk.free()
        x2 = b.linear(o, r + ".attn.out_proj", residual=x, out="f32_strict")
        o.free()
        x.free()
        hn = b.layernorm(x2, r + ".ln_2")
        h1 = b.linear(hn, r + ".mlp.c_fc", act=ACT_QUICKGELU, out="op")
        hn.free()
        x = b.linear(h1, r + ".mlp.c_proj", residual=x2, out="f32_strict")
        h1.free()
        x2.free()
    return x


class ClipTextPlan:
    def __init__(self, b: Builder, *, B, n, width, layers, heads, vocab, embed_dim, normalize=True, prefix="model."):
        self.b = b
        dev = b.device
        self.tokens = torch.zeros(B * n, dtype=torch.int64, device=dev)
        self.eot_rows = torch.zeros(B, dtype=torch.int64, device=dev)        # b * n + argmax(tokens[b]): filled per call
        self.out = torch.zeros(B, embed_dim, dtype=torch.float32, device=dev)
        prog = self.prog = b.new_prog()
        p = prefix
        x = b.f32_strict(B * n, width)
        prog.emit("FRIDO_OP_EMBED", tokens=self.tokens.data_ptr(), tok=b.dev_f32(p + "token_embedding.weight").data_ptr(),
                  pos=b.dev_f32(p + "positional_embedding").data_ptr(), out=x.ptr, rows=B * n, n=n, D=width, vocab=vocab)
        x = resblocks(b, prog, x, p, B=B, n=n, width=width, layers=layers, heads=heads, causal=True)
        xf = b.f32_strict(B * n, width)
        prog.emit("FRIDO_OP_LAYERNORM", x=x.ptr, rows=B * n, C=width, eps=1e-5, weight=b.bias(p + "ln_final.weight"),
                  bias=b.bias(p + "ln_final.bias"), nsplit=b.nsplit, out_f32=xf.ptr, x_bf16=0)
        x.free()
        # the end-of-text token's row of every caption (the highest token id: clip/model.py encode_text), then the projection
        e = b.f32_strict(B, width)
        prog.emit("FRIDO_OP_EMBED", tokens=self.eot_rows.data_ptr(), tok=xf.ptr, pos=None, out=e.ptr, rows=B, n=1, D=width, vocab=B * n)
        xf.free()
        eo = b.pack(e.ptr, 1, B, width, 0, width)
        e.free()
        key = ("clip_proj", p)
        if key not in b._wcache:            # x @ text_projection  ==  Linear with weight text_projection^T
            from .engine import pack_matrix
            b._wcache[key] = pack_matrix(b.w[p + "text_projection"].float().t().contiguous(), b.nsplit)
        z = b.linear(eo, None, wop=b._wcache[key], bias=False, out="f32_strict")
        eo.free()
        if normalize:
            prog.emit("FRIDO_OP_L2NORM", x=z.ptr, out=self.out.data_ptr(), rows=B, C=embed_dim)
        else:
            prog.emit("FRIDO_OP_COPY", src=z.ptr, dst=self.out.data_ptr(), n=rup(B * embed_dim * 4, 16))
        z.free()


class _Rows:
    """A block of f32 rows inside a buffer somebody else owns, as Builder.linear's out=("f32", ...) takes it."""

    def __init__(self, ptr, C):
        self.ptr, self.C = ptr, C


class ClipImagePlan:
    """The image tower of OpenAI CLIP (the `encode_image` path FrozenClipImageEmbedder calls, frido/modules/encoders/modules.py:242-254
    -> clip/model.py VisionTransformer.forward) for one input shape (B, H, W):

        patches = frido_clip_preprocess(x_in)                        [B g^2][3 P^2] f32: resize, normalise, patch cut (csrc/vision.hip;
                                                                     `self.pre`, launched by the caller IN FRONT of the program: no op kind)
        table[1 + i] = PACK(patches)[i] @ conv1.weight.reshape(width, 3 P^2)^T       conv1 has stride = kernel = P and no bias: a Linear
        table[0]     = class_embedding                                               copied once, here: it is a weight
        x[b, j] = table[idx[b, j]] + positional_embedding[j]         (embed kernel; idx[b, 0] = 0, idx[b, 1 + i] = 1 + b g^2 + i, fixed)
        x = ln_pre(x);  layers x ResidualAttentionBlock, no mask     (resblocks: the text tower's ops)
        out = ln_post(x[b, 0]) @ proj                                (row gather, LayerNorm of the B class rows, GEMM); NOT normalised

    `x_in`, `patches`, `out` are fixed buffers, so `pre` + `prog` replay as one captured graph."""

    def __init__(self, b: Builder, *, B, H, W, embed_dim, resolution, layers, width, patch, mean, std, stream, prefix="model.visual."):
        from . import vision
        from .engine import Prog, pack_matrix
        self.b = b
        dev = b.device
        p = prefix
        g = resolution // patch
        n, K, heads = g * g + 1, 3 * patch * patch, width // 64
        self.g, self.n, self.resolution, self.patch = g, n, resolution, patch
        self.x_in = torch.zeros(B, 3, H, W, dtype=torch.float32, device=dev)
        self.patches = b.persistent_f32(B * g * g, K)
        self.pre = vision.preprocess_desc(self.x_in.data_ptr(), self.patches.data_ptr(), B, H, W, resolution, patch, mean, std)
        self.out = torch.zeros(B, embed_dim, dtype=torch.float32, device=dev)
        table = b.persistent_f32(1 + B * g * g, width)
        idx = torch.arange(1, 1 + B * g * g, dtype=torch.int64).view(B, g * g)
        self.idx = torch.cat([torch.zeros(B, 1, dtype=torch.int64), idx], dim=1).reshape(-1).to(dev)
        once = Prog(dev, b.nsplit)
        once.emit("FRIDO_OP_COPY", src=b.dev_f32(p + "class_embedding").data_ptr(), dst=table.data_ptr(), n=width * 4)
        once.run(stream)

        prog = self.prog = b.new_prog()
        # K = 3 P^2 need not be a multiple of the GEMM's 32 (ViT-L/14: 588): PACK zero-fills the operand's columns K .. Cpad and
        # lin_weight -> pack_matrix zero-pads the weight's K on the host to the same Cpad, so the pad contributes exact zeros
        a = b.pack(self.patches.data_ptr(), 1, B * g * g, K, 0, K)
        wop = b.lin_weight(p + "conv1.weight")
        assert a.K == wop.K == rup(K, 32), (a.K, wop.K, K)
        b.linear(a, None, wop=wop, bias=False, out=("f32", _Rows(table.data_ptr() + 4 * width, width)))
        a.free()
        x0 = b.f32_strict(B * n, width)
        prog.emit("FRIDO_OP_EMBED", tokens=self.idx.data_ptr(), tok=table.data_ptr(), pos=b.dev_f32(p + "positional_embedding").data_ptr(),
                  out=x0.ptr, rows=B * n, n=n, D=width, vocab=1 + B * g * g)
        x = b.f32_strict(B * n, width)
        prog.emit("FRIDO_OP_LAYERNORM", x=x0.ptr, rows=B * n, C=width, eps=1e-5, weight=b.bias(p + "ln_pre.weight"),
                  bias=b.bias(p + "ln_pre.bias"), nsplit=b.nsplit, out_f32=x.ptr, x_bf16=0)
        x0.free()
        x = resblocks(b, prog, x, p, B=B, n=n, width=width, layers=layers, heads=heads, causal=False)
        # the class token's row of every image (clip/model.py: ln_post(x[:, 0, :])), then the projection
        self.cls_rows = (torch.arange(B, dtype=torch.int64) * n).to(dev)
        e = b.f32_strict(B, width)
        prog.emit("FRIDO_OP_EMBED", tokens=self.cls_rows.data_ptr(), tok=x.ptr, pos=None, out=e.ptr, rows=B, n=1, D=width, vocab=B * n)
        x.free()
        eo = b.layernorm(e, p + "ln_post")
        e.free()
        key = ("clip_visual_proj", p)
        if key not in b._wcache:            # x @ proj  ==  Linear with weight proj^T
            b._wcache[key] = pack_matrix(b.w[p + "proj"].float().t().contiguous(), b.nsplit)
        b.linear(eo, None, wop=b._wcache[key], bias=False, out=("f32", _Rows(self.out.data_ptr(), embed_dim)))
        eo.free()

    def launch(self, stream):
        """The preprocess kernel, then the program, on `stream` (directly, or inside a capture)."""
        from . import vision
        vision.clip_preprocess(self.pre, stream)
        self.prog.run(stream)
