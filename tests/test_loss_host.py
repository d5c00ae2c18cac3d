"""CPU-side checks of the diffusion objective (FridoDiffusion.forward / p_losses / validation_step): lvlb_weights and the host helpers against
the reference's own tensors (loss_host.npz), the constructor options and state_dict keys, the two launchers in the header and in both
builds, their argument checks (no device is touched), their op kinds in ABI 8, and every refusal with its name."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import golden
from golden_cfg import UNET_SMALL, VQ_SMALL, BERT_SMALL, frido_cfg
from frido_amd import _lib
from frido_amd._lib import FridoHipError


def _model(ucfg=UNET_SMALL, key="crossattn", **over):
    from frido_amd.models import instantiate_from_config
    cfg = frido_cfg(ucfg, VQ_SMALL, BERT_SMALL)
    cfg["cond_stage_config"], cfg["cond_stage_trainable"], cfg["conditioning_key"] = "__is_unconditional__", False, key
    cfg.update(over)
    m = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
    m.model.conditioning_key = key
    return m.eval()


@pytest.fixture(scope="module")
def model():
    return _model()


def test_lvlb_weights_are_bit_identical_to_the_reference(model):
    g = golden("loss_host")
    assert model.lvlb_weights.dtype == torch.float32
    assert np.array_equal(model.lvlb_weights.numpy(), g["lvlb_weights"])
    assert "lvlb_weights" not in model.state_dict()      # non-persistent, like the reference's


def test_host_helpers_match_the_reference(model):
    g = golden("loss_host")
    x, t = torch.from_numpy(g["x"]), torch.from_numpy(g["t"])
    mean, var, logvar = model.q_mean_variance(x, t)
    assert mean.shape == x.shape and var.shape == (3, 1, 1, 1) and logvar.shape == (3, 1, 1, 1)
    assert np.array_equal(mean.numpy(), g["qmv_mean"])
    assert np.array_equal(var.expand_as(x).numpy(), g["qmv_var"]) and np.array_equal(logvar.expand_as(x).numpy(), g["qmv_logvar"])
    assert np.array_equal(model._prior_bpd(x).numpy(), g["prior_bpd"])
    from frido_amd.synth import seeded_normal
    eps = model._predict_eps_from_xstart(x, t, torch.from_numpy(seeded_normal("loss:host:x0", (3, 6, 4, 4))))
    assert np.array_equal(eps.numpy(), g["pred_eps"])


def test_get_loss_is_the_reference_expression():
    a, b = torch.randn(2, 3, 4, 4), torch.randn(2, 3, 4, 4)
    m1, m2 = _model(loss_type="l1"), _model(loss_type="l2")
    assert torch.equal(m1.get_loss(a, b, mean=False), (b - a).abs()) and torch.equal(m1.get_loss(a, b), (b - a).abs().mean())
    assert torch.equal(m2.get_loss(a, b, mean=False), torch.nn.functional.mse_loss(b, a, reduction="none"))
    assert torch.equal(m2.get_loss(a, b), torch.nn.functional.mse_loss(b, a))
    m1.loss_type = "huber"
    with pytest.raises(NotImplementedError, match="unknown loss type"):
        m1.get_loss(a, b)


def test_constructor_keeps_the_objective_options():
    m = _model(loss_type="l2", noise_mix_ratio=0.25, stage_loss_ratio=[0.3, 0.7], l_simple_weight=0.5, original_elbo_weight=0.125,
               learn_logvar=False, logvar_init=-0.5)
    assert (m.loss_type, m.noise_mix_ratio, m.stage_loss_ratio, m.l_simple_weight, m.original_elbo_weight, m.learn_logvar) == \
        ("l2", 0.25, [0.3, 0.7], 0.5, 0.125, False)
    assert not isinstance(m.logvar, torch.nn.Parameter) and m.logvar.shape == (1000,) and bool((m.logvar == -0.5).all())
    with pytest.raises(AssertionError):
        _model(parameterization="x0")


SCHEDULE_KEYS = {"betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
                 "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
                 "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2"}


def test_state_dict_keys_change_only_by_logvar_under_learn_logvar():
    plain, learned = _model(), _model(learn_logvar=True, logvar_init=0.25)
    assert "logvar" not in plain.state_dict() and "lvlb_weights" not in plain.state_dict()
    assert set(learned.state_dict()) - set(plain.state_dict()) == {"logvar"}
    assert set(plain.state_dict()) - set(learned.state_dict()) == set()
    assert isinstance(learned.logvar, torch.nn.Parameter) and bool((learned.logvar == 0.25).all())
    # what a configuration had before this feature it still has, and nothing else: the top-level keys are exactly the schedule
    # buffers of frido.py:127-168 and the scale factor; every other key belongs to the denoiser, its EMA shadow or the first stage
    keys = set(plain.state_dict())
    assert {k for k in keys if "." not in k} == SCHEDULE_KEYS | {"scale_factor"}
    assert {k.split(".")[0] for k in keys if "." in k} == {"model", "model_ema", "first_stage_model"}
    for prefix, module in (("model", plain.model), ("model_ema", plain.model_ema), ("first_stage_model", plain.first_stage_model)):
        assert {k for k in keys if k.startswith(prefix + ".")} == {f"{prefix}.{k}" for k in module.state_dict()}


def test_header_declares_both_launchers_and_their_op_kinds():
    declared = _lib.declared_symbols()
    for name in ("frido_qsample", "frido_diffusion_loss"):
        assert name in declared and name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 8
    assert _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36 and _lib.OP_KINDS["FRIDO_OP_ATTN_MH"] == 26
    assert C.sizeof(_lib.FridoOp) == 520 and C.sizeof(_lib.STRUCTS["FridoGemm"]) == 512
    assert C.sizeof(_lib.STRUCTS["FridoSamplerStep"]) == 232
    assert _lib.OP_KINDS["FRIDO_OP_QSAMPLE"] == 29 and _lib.KIND_STRUCT["FRIDO_OP_QSAMPLE"] == "FridoQSample"
    assert _lib.OP_KINDS["FRIDO_OP_DIFFUSION_LOSS"] == 30 and _lib.KIND_STRUCT["FRIDO_OP_DIFFUSION_LOSS"] == "FridoDiffusionLoss"
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        assert L.frido_abi_version() == 8
        assert L.frido_sizeof_desc(29) == C.sizeof(_lib.STRUCTS["FridoQSample"]) and hasattr(L, "frido_qsample")
        assert L.frido_sizeof_desc(30) == C.sizeof(_lib.STRUCTS["FridoDiffusionLoss"]) and hasattr(L, "frido_diffusion_loss")
    assert C.sizeof(_lib.STRUCTS["FridoQSample"]) == 112 and C.sizeof(_lib.STRUCTS["FridoDiffusionLoss"]) == 120


def test_both_builds_export_both_launchers():
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        assert hasattr(L, "frido_qsample") and hasattr(L, "frido_diffusion_loss"), planes


Q_OK = dict(x0=0x1000, x_noisy=0x2000, t=0x3000, sqrt_ac=0x4000, sqrt_1mac=0x5000, noise=0x6000, B=3, HW=20, Cx=6, ch_start=3, ch_end=6,
            T=1000, mix_tau=0.1)
L_OK = dict(pred=0x1000, t=0x3000, noise=0x6000, logvar=0x4000, lvlb_weights=0x5000, per_sample=0x7000, out=0x8000, B=3, HW=20, Cx=6,
            ch_start=3, nch=3, T=1000, loss_type=1)


@pytest.mark.parametrize("over", [
    dict(x0=None), dict(x_noisy=None), dict(t=None), dict(sqrt_ac=None), dict(sqrt_1mac=None), dict(B=0), dict(B=-1), dict(HW=0), dict(Cx=0),
    dict(T=0), dict(ch_start=-1), dict(ch_start=6), dict(ch_end=7), dict(ch_start=4, ch_end=4),
    dict(noise=None, HW=21, Cx=6),                                        # Philox groups of 4 floats
    dict(Cx=8, ch_start=4, ch_end=8, x0=0x1004), dict(Cx=8, ch_start=4, ch_end=8, x_noisy=0x2008), dict(Cx=8, ch_start=0, ch_end=4, noise=0x6004),
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_qsample_rejects_bad_descriptors_without_touching_a_device(over):
    L = _lib.lib()
    d = _lib.STRUCTS["FridoQSample"](**dict(Q_OK, **over))
    assert L.frido_qsample(C.byref(d), None) == -1, over
    assert b"frido_qsample" in L.frido_last_error()


@pytest.mark.parametrize("over", [
    dict(pred=None), dict(per_sample=None), dict(t=None), dict(logvar=None), dict(lvlb_weights=None), dict(T=0), dict(B=0), dict(HW=-2),
    dict(Cx=0), dict(nch=0), dict(ch_start=-1), dict(ch_start=4), dict(nch=7, ch_start=0), dict(loss_type=2), dict(loss_type=-1),
    dict(noise=None, HW=21),
    dict(Cx=8, ch_start=4, nch=4, pred=0x1008), dict(Cx=8, ch_start=0, nch=4, noise=0x6004),
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_diffusion_loss_rejects_bad_descriptors_without_touching_a_device(over):
    L = _lib.lib()
    d = _lib.STRUCTS["FridoDiffusionLoss"](**dict(L_OK, **over))
    assert L.frido_diffusion_loss(C.byref(d), None) == -1, over
    assert b"frido_diffusion_loss" in L.frido_last_error()


def test_null_descriptors_are_rejected():
    L = _lib.lib()
    assert L.frido_qsample(None, None) == -1 and b"frido_qsample" in L.frido_last_error()
    assert L.frido_diffusion_loss(None, None) == -1 and b"frido_diffusion_loss" in L.frido_last_error()


def test_objective_launchers_are_op_kinds_for_captured_programs():
    d = _lib.STRUCTS["FridoQSample"](**Q_OK)
    assert _lib.op_of("FRIDO_OP_QSAMPLE", d) == (29, d) and _lib.op_of("FRIDO_OP_DIFFUSION_LOSS", _lib.STRUCTS["FridoDiffusionLoss"](**L_OK))[0] == 30
    assert _lib.make_op("FRIDO_OP_UNFOLD")[0] == 27 and _lib.make_op("FRIDO_OP_FOLD")[0] == 28
    with pytest.raises(TypeError, match="FRIDO_OP_DIFFUSION_LOSS takes a FridoDiffusionLoss"):
        _lib.op_of("FRIDO_OP_DIFFUSION_LOSS", d)


# ---- refusals: by name, never ignored -------------------------------------------------------------------------------------------------
X, CTX, TT = torch.zeros(2, 6, 16, 16), torch.zeros(2, 5, 64), torch.tensor([1, 2])


def test_cpu_tensors_raise_the_hip_error(model, monkeypatch):
    with pytest.raises(FridoHipError, match="no CPU fallback"):
        model(X, CTX)
    with pytest.raises(FridoHipError, match="no CPU fallback"):
        model.p_losses(X, CTX, TT, 0)
    monkeypatch.setattr(model, "get_input", lambda batch, k: [batch["z"], batch["c"]], raising=False)
    with pytest.raises(FridoHipError, match="no CPU fallback"):
        model.validation_step(dict(z=X, c=CTX), 0)


def test_training_step_says_there_is_no_backward_pass(model):
    with pytest.raises(FridoHipError, match="no backward pass"):
        model.training_step({}, 0)


def test_split_input_params_is_refused():
    m = _model()
    m.split_input_params = dict(ks=(8, 8), stride=(4, 4))
    for call in (lambda: m(X, CTX), lambda: m.p_losses(X, CTX, TT, 0)):
        with pytest.raises(NotImplementedError, match="split_input_params"):
            call()


def test_shorten_cond_schedule_is_refused():
    m = _model(num_timesteps_cond=2)
    assert m.shorten_cond_schedule
    with pytest.raises(NotImplementedError, match="shorten_cond_schedule"):
        m(X, CTX)


@pytest.mark.parametrize("cond", [dict(c_crossattn=[CTX]), [CTX]], ids=["dict", "list"])
def test_dict_and_list_conditionings_are_refused(model, cond):
    with pytest.raises(NotImplementedError, match="dict / list conditionings"):
        model(X, cond)
    with pytest.raises(NotImplementedError, match="dict / list conditionings"):
        model.p_losses(X, cond, TT, 1)


@pytest.mark.parametrize("key", ["concat", "hybrid"])
def test_concat_and_hybrid_keys_are_refused(key):
    m = _model(key=key)
    with pytest.raises(NotImplementedError, match=f"conditioning_key='{key}'"):
        m(X, CTX)


def test_a_denoiser_without_the_split_head_is_refused():
    m = _model(ucfg=dict(UNET_SMALL, use_split_head=False, split_embed_dim_list=[], use_SPADE_norm=False, num_stage=1))
    with pytest.raises(NotImplementedError, match="use_split_head=False"):
        m(X, CTX)


def test_forward_takes_no_stray_arguments(model):
    with pytest.raises(TypeError, match="unexpected arguments"):
        model(X, CTX, 3)
