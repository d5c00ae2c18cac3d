"""The patch-wise mode (FridoDiffusion.split_input_params) on the MI355X against goldens captured from the reference's own patch-wise
branches (tests/golden/make_golden_patch.py): apply_model eps at both stages with tie_braker both ways and on a rectangular latent, DDIM /
PLMS sampling, patch-wise decode and encode of the first stage; replay against the eager path, repeatability, and the whole-latent
results with the attribute deleted again.

Bounds are the ones tests/test_model_gpu.py uses for the same arithmetic: forward eps and decoded image 2e-4
(test_unet_forward_matches_reference_golden, the decode goldens), sampled latents 1e-3 (test_sampler_matches_reference_golden; every run's
*_ref_sens is asserted below 1e-4), encode in the form of test_vq_encode_matches_reference_golden.  The patch-wise result differs from the
whole-latent one by O(1) (*_whole_minus_patch in the fixtures), so these comparisons fail wherever the attribute is ignored.
A FridoNumericsWarning is an error here.
"""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import golden  # noqa: E402
from golden_cfg import VQ_SMALL, BERT_SMALL, frido_cfg  # noqa: E402
from patch_cfg import MODELS, SPLIT, SPLIT_TIE, SPLIT_RECT, SPLIT_ENC, COND_STAGE_KEY, RUNS  # noqa: E402
from frido_amd.synth import fill_module  # noqa: E402


@pytest.fixture(autouse=True)
def _no_numerics_warning():
    from frido_amd import _lib
    _lib.status_flags(clear=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", _lib.FridoNumericsWarning)
        yield
    assert _lib.status_flags(clear=True) == 0


def _rel(got, ref):
    ref = torch.as_tensor(ref).double()
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


_MODELS = {}


def _frido(mname, scale_factor=(0.9, 1.1)):
    """One model per (denoiser, scale factors) for the module; every test leaves it WITHOUT split_input_params."""
    key = (mname, scale_factor)
    if key not in _MODELS:
        from frido_amd.models import instantiate_from_config
        cfg = dict(frido_cfg(MODELS[mname], VQ_SMALL, BERT_SMALL), cond_stage_key=COND_STAGE_KEY)
        cfg["cond_stage_config"], cfg["conditioning_key"] = "__is_unconditional__", "crossattn"      # the conditioning tensor is fed directly
        m = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
        m.model.conditioning_key = "crossattn"      # ('__is_unconditional__' resets the wrapper's key to None, like the reference)
        fill_module(m.model, "model.")
        fill_module(m.first_stage_model, "first_stage_model.")
        m.scale_factor.copy_(torch.tensor(scale_factor))
        _MODELS[key] = m.cuda().eval()
    m = _MODELS[key]
    assert not hasattr(m, "split_input_params")
    return m


class _split:
    def __init__(self, model, params):
        self.model, self.params = model, params

    def __enter__(self):
        self.model.split_input_params = dict(self.params)
        return self.model

    def __exit__(self, *a):
        del self.model.split_input_params


@pytest.mark.parametrize("mname,tname", [pytest.param("spade", "notie", marks=pytest.mark.gate), ("spade", "tie"), ("plain", "notie"),
                                         ("plain", "tie")])
def test_apply_model_matches_reference_golden(mname, tname):
    g = golden("patch_apply")
    assert float(g[f"{mname}_whole_minus_patch"]) > 1.0      # what ignoring the attribute would cost
    m = _frido(mname)
    x, t, c = (torch.from_numpy(g[k]).cuda() for k in ("x", "t", "c"))
    whole = m.apply_model(x, t, c, stage=1)
    with _split(m, SPLIT_TIE if tname == "tie" else SPLIT):
        for s in range(2):
            e = m.apply_model(x[:, :3 * (s + 1)].contiguous(), t, c, stage=s)
            ref = g[f"{mname}_{tname}_eps_{s}"]
            assert e.shape == ref.shape
            err = _rel(e, ref)
            print(f"{mname} {tname} stage {s}: patch-wise eps max-relative error {err:.3e}")
            assert err < 2e-4, (mname, tname, s)
        again = m.apply_model(x, t, c, stage=1)
        assert torch.equal(again, e)                          # a second call: the same bits
        assert float((e - whole).abs().max()) > 0.5           # and not the whole-latent result
    # the attribute deleted: the whole-latent result again, bit for bit
    assert torch.equal(m.apply_model(x, t, c, stage=1), whole)


def test_apply_model_on_a_rectangular_latent_matches_reference_golden():
    g = golden("patch_apply")
    m = _frido("spade")
    x, t, c = (torch.from_numpy(g[k]).cuda() for k in ("xr", "t", "c"))
    with _split(m, SPLIT_RECT):
        for s in range(2):
            e = m.apply_model(x[:, :3 * (s + 1)].contiguous(), t, c, stage=s)
            err = _rel(e, g[f"rect_eps_{s}"])
            print(f"12 x 20 latent, 4 x 8 crops, stage {s}: eps max-relative error {err:.3e}")
            assert e.shape == g[f"rect_eps_{s}"].shape and err < 2e-4, s


def _sample(model, g, run, c):
    from frido.models.diffusion.ddim import DDIMSampler
    from frido.models.diffusion.plms import PLMSSampler
    S, eta, scale, lev = g[f"{run}_args"]
    cls = PLMSSampler if RUNS[run][1] == "plms" else DDIMSampler
    torch.manual_seed(23)           # noise="torch": the host generator's stream, draw for draw the reference's CPU run
    return cls(model).sample(S=int(S), batch_size=2, shape=(6, 16, 16), conditioning=c, num_stage=2, eta=float(eta), verbose=False,
                             log_every_t=int(lev), unconditional_guidance_scale=float(scale),
                             unconditional_conditioning=torch.zeros_like(c) if scale != 1.0 else None, noise="torch")


def _patch_engines(model):
    return [e for e in model.model.diffusion_model.runtime().__dict__.get("_sampler_engines", {}).values() if e.geo is not None]


@pytest.mark.parametrize("run", [pytest.param("ddim_eta1", marks=pytest.mark.gate), "plms", "ddim_eta0_cfg"])
def test_sampler_matches_reference_golden_and_replays_the_eager_path(run):
    g = golden("patch_sampler")
    assert float(g[f"{run}_ref_sens"]) < 1e-4              # the fixture is well conditioned (patch_cfg.py)
    assert float(g[f"{run}_whole_minus_patch"]) > 0.1      # what ignoring the attribute would cost
    mname, _, _, _, _, split = RUNS[run]
    model = _frido(mname)
    c = torch.from_numpy(g["c"]).cuda()
    whole, _ = _sample(model, g, run, c)
    with _split(model, split):
        samples, inter = _sample(model, g, run, c)
        err = _rel(samples, g[f"{run}_samples"])
        print(f"{run}: patch-wise latent max-relative error {err:.3e} (the whole-latent run is {_rel(whole, g[f'{run}_samples']):.2e} away)")
        assert err < 1e-3
        assert len(inter["x_inter"]) == int(g[f"{run}_nx"])
        assert _rel(inter["x_inter"][-1], g[f"{run}_x_inter_last"]) < 1e-3
        assert _rel(inter["pred_x0"][1], g[f"{run}_pred_x0_1"]) < 1e-3
        # a second run replays the captured graphs: identical bits
        eng = _patch_engines(model)[-1]      # most recently used: this run's (the model is shared, earlier runs' engines may be cached too)
        assert eng.kind == RUNS[run][1] and eng.graphs
        again, _ = _sample(model, g, run, c)
        assert torch.equal(again, samples)
        # the same step bodies run eagerly (unfold, frido_run segments, fold launched one by one): identical bits
        eng.use_graph, eng.graphs = False, {}
        try:
            eager, _ = _sample(model, g, run, c)
        finally:
            eng.use_graph, eng.graphs = True, {}
        assert torch.equal(eager, samples)
    # the attribute deleted: the whole-latent engine and its bits again
    after, _ = _sample(model, g, run, c)
    assert torch.equal(after, whole) and _rel(whole, g[f"{run}_samples"]) > 0.1


def test_multi_step_patch_graph_equals_the_eager_path(monkeypatch):
    """The K-step graph (the step body K times in one captured graph, sharing the unfold / fold descriptors) is what long runs replay.  With
    K lowered to 2 the four-step fixture run replays it once (steps 1-2; steps 0 and 3 touch the host for the log); the result is the golden's,
    and the eager path's bit for bit."""
    from frido_amd import runtime
    monkeypatch.setattr(runtime, "GRAPH_STEPS", 2)
    run = "ddim_eta1"
    g = golden("patch_sampler")
    model = _frido(RUNS[run][0])
    c = torch.from_numpy(g["c"]).cuda()
    gl = {k: (np.array([4, 1.0, 1.0, 100.0]) if k == f"{run}_args" else g[k]) for k in g.files}      # nothing logged in between
    with _split(model, RUNS[run][5]):
        samples, _ = _sample(model, gl, run, c)
        eng = _patch_engines(model)[-1]
        assert eng.kind == "ddim" and getattr(eng, "multi_step_launches", 0) >= 2      # once per stage
        assert any(len(k) == 3 and k[2] == "x2" for k in eng.graphs)
        assert _rel(samples, g[f"{run}_samples"]) < 1e-3
        launches = eng.multi_step_launches
        eng.use_graph, eng.graphs = False, {}
        try:
            eager, _ = _sample(model, gl, run, c)
        finally:
            eng.use_graph, eng.graphs = True, {}
        assert eng.multi_step_launches == launches and torch.equal(eager, samples)


def _np_u8(x):      # scripts/sample_diffusion.py:115-121 custom_to_np
    return ((x.detach().cpu() + 1) * 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _pil_u8(x):     # scripts/sample_diffusion.py:103-113 custom_to_pil
    v = ((torch.clamp(x.detach().cpu(), -1., 1.) + 1.) / 2.).permute(0, 2, 3, 1).contiguous()
    return torch.from_numpy((255 * v.numpy()).astype(np.uint8))


def test_patch_decode_matches_reference_golden():
    g, gv = golden("patch_vq"), golden("vq_small")
    m = _frido("spade", (1.0, 1.0))
    h = torch.from_numpy(gv["h"]).cuda()
    whole = m.decode_first_stage(h)
    with _split(m, SPLIT):
        dec = m.decode_first_stage(h)
        err = _rel(dec, g["dec"])
        print(f"patch-wise decode: max-relative error {err:.3e} (whole decode: {_rel(whole, g['dec']):.2e} away)")
        assert dec.shape == g["dec"].shape and err < 2e-4
        assert torch.equal(m.decode_first_stage(h), dec)
        assert torch.equal(m.decode_first_stage(h, to_uint8=True).cpu(), _np_u8(dec))
        assert torch.equal(m.decode_first_stage(h, to_uint8="pil").cpu(), _pil_u8(dec))
    with _split(m, dict(SPLIT, patch_distributed_vq=False)):       # frido.py:878-882: the whole latent
        assert torch.equal(m.decode_first_stage(h), whole)
    assert torch.equal(m.decode_first_stage(h), whole) and _rel(whole, gv["dec"]) < 2e-4


def test_patch_encode_matches_reference_golden():
    g, gv = golden("patch_vq"), golden("vq_small")
    m = _frido("spade", (1.0, 1.0))
    img = torch.from_numpy(gv["img"]).cuda()
    whole = m.encode_first_stage(img)
    with _split(m, SPLIT_ENC):
        enc = m.encode_first_stage(img)
        assert tuple(m.split_input_params["original_image_size"]) == (64, 64)
        assert enc.shape == g["enc"].shape
        # the bound form of test_vq_encode_matches_reference_golden: the coarse scale is quantised on the way to the fine one
        err = (enc.cpu() - torch.from_numpy(g["enc"])).abs()
        scale = float(np.abs(g["enc"]).max())
        print(f"patch-wise encode: coarse max error {float(err[:, :3].max()) / scale:.3e}, fine pixels over 5e-4: {float((err > 5e-4 * scale).float().mean()):.4f}")
        assert float((err > 5e-4 * scale).float().mean()) < 0.02
        assert float(err[:, :3].max()) < 5e-4 * scale
        assert torch.equal(m.encode_first_stage(img), enc)
    assert torch.equal(m.encode_first_stage(img), whole) and float((whole.cpu() - torch.from_numpy(g["enc"])).abs().max()) > 0.5
