"""Records the exact bits of the Python front end over the HIP programs -- the first-stage classes and DecoderRuntime, the patch-wise
decode / encode, the two text towers, the objective on LossEngine and PyUNetModel.forward with its runtime swaps -- on an MI355X, from
whichever checkout --repo names, into an .npz: the fixture of tests/test_frontend_bits_gpu.py.

    python tests/golden/record_frontend_bits.py --repo <built checkout of the commit to pin> --out tests/golden/frontend_bits.npz

tests/golden/frontend_bits.npz was recorded this way from a built checkout of fd7ac4f, the last commit before the plumbing between the
public classes and the programs (runtime(), the first-stage and text-tower bases, DecoderRuntime's plan getters and patch hand-offs, the
stream hand-over and the LRU) was folded; two recordings were identical.  Every GEMM runs on the library's static tile (FRIDO_TUNE = 0
here, tune.ENABLED = False in the test).  Inputs are synth.seeded_normal streams; the host generator is seeded where the objective draws.

  first_stage  VQModelInterface on VQ_SMALL, B = 2, 64 x 64 images (latents 8 x 8 and 16 x 16): decode (f32, to_uint8 "np" / "pil",
               return_code, force_codes, an inv_scale), encode with and without scale
  msvq         MSFPNVQModel: encode, decode, forward with and without use_aux_loss (twice each: capture, then replay), log_images
  patch        decode_first_stage / encode_first_stage under patch_cfg.SPLIT / SPLIT_ENC (f32 and uint8 decode), then a whole-latent call at
               the crop size on the same runtime (the plan both share), and the other order on a fresh runtime
  cond         BERTEmbedder on BERT_SMALL ids at two (B, n) shapes, the first again after five other shapes (evicted and rebuilt);
               FrozenCLIPTextEmbedder with the reduced arch of tests/test_model_gpu.py, forward and encode
  objective    p_losses per stage and forward on the small two-stage model, Philox noise, a host tape, the host generator; nine
               noise_mix_ratio values (LossEngine keeps 8 graphs: one goes) and the first again
  denoiser     PyUNetModel.forward per stage; stage 1 inside ema_scope(keep_runtimes=True), after it, and inside a second scope

An entry of at most FULL values is stored as it is (float32 / int64); anything larger as the SHA-256 of its tensors' bytes (32 uint8), so
the file stays far below 1 MiB; every float tensor is checked to be finite before it is stored or hashed.  `runs(group)` is shared with
the test: only public names that exist on both sides of the change.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

SEED, B, FULL = 11, 2, 64
GROUPS = ("first_stage", "msvq", "patch", "cond", "objective", "denoiser")
DUMMY = dict(target="taming.modules.losses.DummyLoss")
CLIP_ARCH = (64, 16, 1000, 128, 4, 3)
MIX = (0.0, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4)
# entries that differ in one option must differ in bits.  (Not "np" against "pil": (x + 1) * 127.5 and 255 * ((x + 1) * 0.5) are the same real
# product rounded once -- the halving is exact -- and both clamps cut at the same x, so the two conversions agree on every finite value.)
DIFFERENT = (("first_stage.dec", "first_stage.dec_np"), ("first_stage.dec", "first_stage.dec_inv"),
             ("first_stage.dec", "first_stage.dec_forced"), ("first_stage.enc", "first_stage.enc_scaled"),
             ("msvq.fwd.1", "msvq.fwd_aux.1"), ("msvq.log", "msvq.log_aux"), ("patch.dec", "patch.dec_u8"), ("patch.dec", "patch.whole_dec"),
             ("cond.bert.a", "cond.bert.b"), ("cond.clip.forward", "cond.clip.encode"),
             ("objective.p_losses.philox.s0", "objective.p_losses.philox.s1"), ("objective.p_losses.philox.s0", "objective.p_losses.tape.s0"),
             ("objective.forward.philox", "objective.forward.tape"), ("objective.mix0", "objective.mix8"),
             ("denoiser.s0", "denoiser.s1"), ("denoiser.s1", "denoiser.ema_in"))
_MODELS = {}


def _normal(tag, shape):
    import torch
    from frido_amd.synth import seeded_normal
    return torch.from_numpy(seeded_normal("frontend_bits:" + tag, shape))


def _ids(tag, shape, vocab):
    import torch
    from frido_amd.synth import seeded_normal
    return torch.from_numpy((np.abs(seeded_normal("frontend_bits:" + tag, shape)) * 1000).astype(np.int64) % vocab)


def _arrays(v):
    """The arrays of a tensor, a number, a host list of code lists or any nesting of them, in order; None is skipped."""
    import torch
    if v is None:
        return []
    if torch.is_tensor(v):
        a = v.detach().cpu()
        a = a.float().numpy() if a.is_floating_point() else a.numpy()
    elif isinstance(v, dict):
        return [a for k in sorted(v) for a in _arrays(v[k])]
    elif isinstance(v, (list, tuple)) and any(torch.is_tensor(e) or isinstance(e, (list, tuple, dict)) or e is None for e in v):
        return [a for e in v for a in _arrays(e)]
    else:
        a = np.asarray(v)
        assert a.dtype.kind in "fiu", a.dtype
    a = np.ascontiguousarray(a)
    assert a.dtype.kind != "f" or np.isfinite(a).all()
    return [a]


def _put(out, name, *values):
    arrs = _arrays(values)
    assert arrs, name
    if sum(a.size for a in arrs) <= FULL and len({a.dtype.kind for a in arrs}) == 1:
        out[name] = np.concatenate([a.reshape(-1) for a in arrs]).astype(np.float32 if arrs[0].dtype.kind == "f" else np.int64)
        return
    h = hashlib.sha256()
    for a in arrs:
        h.update(repr((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    out[name] = np.frombuffer(h.digest(), dtype=np.uint8).copy()


def model_of(name):
    """"vq" / "msvq" / "msvq_aux": the first-stage classes on VQ_SMALL; "bert" / "clip": the text towers; "frido": the small two-stage
    model of record_sampler_bits.build_model() with a conditioning tensor fed directly -> (model, context)."""
    if name not in _MODELS:
        from golden_cfg import VQ_SMALL, BERT_SMALL
        from frido_amd import models
        from frido_amd.synth import fill_module
        if name == "vq":
            m = fill_module(models.VQModelInterface(**VQ_SMALL, lossconfig=DUMMY), "first_stage_model.").cuda().eval()
        elif name in ("msvq", "msvq_aux"):
            m = fill_module(models.MSFPNVQModel(**dict(VQ_SMALL, lossconfig=DUMMY, use_aux_loss=name == "msvq_aux")), "first_stage_model.").cuda().eval()
        elif name == "bert":
            m = fill_module(models.BERTEmbedder(**BERT_SMALL), "cond_stage_model.").cuda()
        elif name == "clip":
            m = fill_module(models.FrozenCLIPTextEmbedder(n_repeat=3, arch=CLIP_ARCH), "cond_stage_model.").cuda()
        else:
            import record_sampler_bits
            m, c = record_sampler_bits.build_model()
            m.model.conditioning_key = "crossattn"      # ('__is_unconditional__' resets the wrapper's key to None, like the reference)
            m.cond_stage_trainable = False      # the context is the finished conditioning (no cond stage model to run it through)
            m = (m, c)
        _MODELS[name] = m
    return _MODELS[name]


class _split:
    def __init__(self, model, params):
        self.model, self.params = model, params

    def __enter__(self):
        self.model.split_input_params = dict(self.params)

    def __exit__(self, *a):
        del self.model.split_input_params


def _first_stage(out):
    v = model_of("vq")
    z, z2, img = _normal("z", (B, 6, 16, 16)).cuda(), _normal("z2", (B, 6, 16, 16)).cuda(), _normal("img", (B, 3, 64, 64)).cuda()
    _put(out, "first_stage.dec", v.decode(z))
    _put(out, "first_stage.dec_np", v.decode(z, to_uint8="np"))
    _put(out, "first_stage.dec_pil", v.decode(z, to_uint8="pil"))
    dec, codes = v.decode(z2, return_code=True)
    _put(out, "first_stage.dec_code", dec, codes)
    _put(out, "first_stage.dec_forced", v.decode(z, force_codes=codes))
    _put(out, "first_stage.dec_inv", v.decode(z, inv_scale=[1.0 / 0.9, 1.0 / 1.1]))
    _put(out, "first_stage.dec_again", v.decode(z))
    _put(out, "first_stage.enc", v.encode(img))
    _put(out, "first_stage.enc_scaled", v.encode(img, scale=[0.9, 1.1]))


def _msvq(out):
    m, ma = model_of("msvq"), model_of("msvq_aux")
    img = _normal("img", (B, 3, 64, 64)).cuda()
    quant, loss, info = m.encode(img)
    _put(out, "msvq.enc", quant, loss, info)
    _put(out, "msvq.enc_loss", loss)
    _put(out, "msvq.dec", m.decode(quant))
    _put(out, "msvq.dec_u8", m.decode(quant, to_uint8=True))
    for k in (1, 2):
        _put(out, f"msvq.fwd.{k}", m(img))
        _put(out, f"msvq.fwd_aux.{k}", ma(img))
    batch = dict(image=img.permute(0, 2, 3, 1).contiguous(), file_name=["a", "b"])
    for name, mod in (("msvq.log", m), ("msvq.log_aux", ma)):
        log = mod.log_images(batch)
        assert log.pop("file_name") == ["a", "b"]
        _put(out, name, log)


def _patch(out):
    from patch_cfg import SPLIT, SPLIT_ENC
    model, _ = model_of("frido")
    fs = model.first_stage_model
    z, img = _normal("z", (B, 6, 16, 16)).cuda(), _normal("img", (B, 3, 64, 64)).cuda()
    zc, imgc = _normal("zc", (B * 9, 6, 8, 8)).cuda(), _normal("imgc", (B * 9, 3, 32, 32)).cuda()     # whole inputs of the crops' size and batch

    def patch_first(sfx):
        with _split(model, SPLIT):
            _put(out, "patch.dec" + sfx, model.decode_first_stage(z))
            _put(out, "patch.dec_u8" + sfx, model.decode_first_stage(z, to_uint8=True))
        _put(out, "patch.whole_dec" + sfx, model.decode_first_stage(zc))
        with _split(model, SPLIT_ENC):
            _put(out, "patch.enc" + sfx, model.encode_first_stage(img))
        _put(out, "patch.whole_enc" + sfx, model.encode_first_stage(imgc))

    def whole_first(sfx):
        _put(out, "patch.whole_dec" + sfx, model.decode_first_stage(zc))
        _put(out, "patch.whole_enc" + sfx, model.encode_first_stage(imgc))
        with _split(model, SPLIT):
            _put(out, "patch.dec" + sfx, model.decode_first_stage(z))
            _put(out, "patch.dec_u8" + sfx, model.decode_first_stage(z, to_uint8=True))
        with _split(model, SPLIT_ENC):
            _put(out, "patch.enc" + sfx, model.encode_first_stage(img))

    fs.invalidate()
    patch_first("")
    fs.invalidate()      # a fresh runtime: the whole-latent call builds the shared plan this time
    whole_first(".whole_first")


def _cond(out):
    from golden_cfg import BERT_SMALL
    bert, clip = model_of("bert"), model_of("clip")
    vocab = BERT_SMALL["vocab_size"]
    bert.invalidate()
    a, b = _ids("bert_a", (2, 16), vocab).cuda(), _ids("bert_b", (3, 9), vocab).cuda()
    _put(out, "cond.bert.a", bert(a))
    _put(out, "cond.bert.b", bert.encode(b))
    z, tok = bert(a, return_token=True)
    _put(out, "cond.bert.a_token", z, tok)
    for k, shape in enumerate(((1, 4), (1, 5), (2, 6), (2, 7), (3, 8))):
        _put(out, f"cond.bert.other{k}", bert(_ids(f"bert_o{k}", shape, vocab).cuda()))
    _put(out, "cond.bert.a_rebuilt", bert(a))
    ctx, cv = CLIP_ARCH[1], CLIP_ARCH[2]
    t = _ids("clip", (3, ctx), cv - 2)
    for r, n in enumerate((3, 9, 13)):      # rows like clip.tokenize's: SOT, words, EOT (the highest id), zero padding
        t[r, 0], t[r, n], t[r, n + 1:] = cv - 2, cv - 1, 0
    _put(out, "cond.clip.forward", clip(t.cuda()))
    _put(out, "cond.clip.encode", clip.encode(t.cuda()))
    _put(out, "cond.clip.forward_short", clip(t[:2, :14].cuda()))


def _objective(out):
    import torch
    model, c = model_of("frido")
    x, t = _normal("x0", (B, 6, 16, 16)).cuda(), torch.tensor([17, 903])
    tape = [_normal(f"noise{s}", (B, 6, 16, 16)) for s in range(2)]
    keep = model.noise_mix_ratio
    try:
        for s in range(2):
            _put(out, f"objective.p_losses.philox.s{s}", model.p_losses(x, c, t, s, noise="philox", seed=SEED, sample0=3, return_per_sample=True))
            _put(out, f"objective.p_losses.tape.s{s}", model.p_losses(x, c, t, s, noise=tape[s], return_per_sample=True))
            torch.manual_seed(SEED)
            _put(out, f"objective.p_losses.torch.s{s}", model.p_losses(x, c, t, s))
        _put(out, "objective.forward.philox", model(x, c, t=t, noise="philox", seed=SEED))
        _put(out, "objective.forward.tape", model(x, c, t=t.cuda(), noise=tape[0]))
        torch.manual_seed(SEED)
        _put(out, "objective.forward.torch", model(x, c))      # t = randint first, then one randn per stage
        for k, mix in enumerate(MIX + MIX[:1]):
            model.noise_mix_ratio = mix
            _put(out, f"objective.mix{k}", model(x, c, t=t, noise="philox", seed=SEED))
    finally:
        model.noise_mix_ratio = keep


def _denoiser(out):
    import torch
    from loss_cfg import ema_shadow
    model, c = model_of("frido")
    unet = model.model.diffusion_model
    x, t = _normal("x", (B, 6, 16, 16)).cuda(), torch.tensor([17, 903]).cuda()
    params = dict(model.model.named_parameters())
    names = {s: k for k, s in model.model_ema.m_name2s_name.items()}
    with torch.no_grad():
        for s_name, buf in model.model_ema.named_buffers():
            if s_name in names:
                buf.copy_(torch.from_numpy(ema_shadow(names[s_name], params[names[s_name]].detach().cpu().numpy())))
    _put(out, "denoiser.s0", unet(x[:, :3].contiguous(), t, context=c, stage=0))
    _put(out, "denoiser.s1", unet(x, t, context=c, stage=1))
    with model.ema_scope(keep_runtimes=True):
        _put(out, "denoiser.ema_in", unet(x, t, context=c, stage=1))
    _put(out, "denoiser.after", unet(x, t, context=c, stage=1))
    with model.ema_scope(keep_runtimes=True):
        _put(out, "denoiser.ema_in2", unet(x, t, context=c, stage=1))
    with model.ema_scope():
        _put(out, "denoiser.ema_plain", unet(x, t, context=c, stage=1))
    _put(out, "denoiser.after_plain", unet(x, t, context=c, stage=1))


def runs(group):
    """{name: array} of one group of GROUPS."""
    out = {}
    dict(first_stage=_first_stage, msvq=_msvq, patch=_patch, cond=_cond, objective=_objective, denoiser=_denoiser)[group](out)
    assert out and all(k.startswith(group + ".") for k in out)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repo", required=True, help="built checkout whose frido_amd is recorded")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    os.environ["FRIDO_TUNE"] = "0"
    repo = os.path.abspath(a.repo)
    sys.path[:0] = [repo, os.path.join(repo, "tests", "golden")]
    import frido_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(frido_amd.__file__))) == repo, frido_amd.__file__
    res = {}
    for group in GROUPS:
        res.update(runs(group))
    same = [(a_, b_) for a_, b_ in DIFFERENT if np.array_equal(res[a_], res[b_])]
    assert not same, same
    np.savez_compressed(a.out, **res)
    print({k: v.tolist() for k, v in res.items() if v.dtype != np.uint8})
    print(sorted(res))
