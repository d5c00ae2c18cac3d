"""CPU-side checks of ancestral (DDPM) sampling: the posterior schedule tables against the reference's own buffers (anc_tables.npz), the
loop-order coefficient rows of the update kernel, the public methods' signatures, the unchanged descriptor layout (ABI 8 now) with the new hist_mode
value, the launcher's argument checks (no device is touched), and the options that are refused by name."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from helpers import golden
from golden_cfg import VQ_SMALL, BERT_SMALL, frido_cfg
from ancestral_cfg import AB_SMP, TABLES, LINEAR, POSTERIOR_KEYS, SIGNATURES
from frido_amd import _lib, schedules


def _tables(tag):
    sched, T, v = TABLES[tag]
    return schedules.ddpm_tables(schedules.make_beta_schedule(sched, T, **LINEAR), v_posterior=v), T


@pytest.mark.parametrize("tag", sorted(TABLES))
def test_posterior_tables_are_bit_identical_to_the_reference(tag):
    g = golden("anc_tables")
    tabs, T = _tables(tag)
    for k in POSTERIOR_KEYS:
        assert tabs[k].dtype == np.float32 and tabs[k].shape == (T,)
        assert np.array_equal(tabs[k], g[f"{tag}_{k}"]), (tag, k)


@pytest.mark.parametrize("tag,T", [("linear1000", None), ("linear1000", 12), ("cosine20", None), ("cosine20", 1)])
def test_ancestral_table_rows_are_the_buffers_in_loop_order(tag, T):
    g = golden("anc_tables")
    tabs, n = _tables(tag)
    for clip in (False, True):
        tab = schedules.ancestral_table(tabs, T, clip_denoised=clip)
        T_ = n if T is None else T
        assert tab.shape == (T_, schedules.COEF_ROW) and tab.dtype == np.float32
        t = np.arange(T_ - 1, -1, -1)
        for col, k in enumerate(("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2")):
            assert np.array_equal(tab[:, col], g[f"{tag}_{k}"][t]), k
        sigma = torch.exp(0.5 * torch.from_numpy(g[f"{tag}_posterior_log_variance_clipped"][t])).numpy()      # frido.py:1305, fp32
        assert np.allclose(tab[:-1, 4], sigma[:-1], rtol=2e-7, atol=0) and tab[-1, 4] == 0.0               # nonzero_mask: exactly 0 at t = 0
        assert np.all(tab[:, 5] == (1.0 if clip else 0.0)) and np.all(tab[:, 6:] == 0.0)
    with pytest.raises(AssertionError):
        schedules.ancestral_table(tabs, n + 1)


def _model(ucfg=AB_SMP, **over):
    from frido_amd.models import instantiate_from_config
    cfg = dict(frido_cfg(ucfg, VQ_SMALL, BERT_SMALL), **over)
    cfg["cond_stage_config"], cfg["cond_stage_trainable"], cfg["conditioning_key"] = "__is_unconditional__", False, None
    return instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))


def test_model_registers_the_posterior_buffers_and_honours_v_posterior():
    g = golden("anc_tables")
    m = _model()
    sd = m.state_dict()
    for k in POSTERIOR_KEYS:
        assert k in sd and torch.equal(sd[k], torch.from_numpy(g[f"linear1000_{k}"])), k
    mv = _model(v_posterior=0.25)
    for k in POSTERIOR_KEYS:
        assert torch.equal(getattr(mv, k), torch.from_numpy(g[f"linear1000_v_{k}"])), k
    assert m.clip_denoised is False      # frido.py:540: FridoDiffusion.__init__ resets it whatever the keyword says


def test_public_methods_have_the_reference_parameter_names():
    from frido_amd.models import FridoDiffusion
    for name, want in SIGNATURES.items():
        ps = inspect.signature(getattr(FridoDiffusion, name)).parameters
        got = [p for p, v in ps.items() if p not in ("self", "kwargs") and v.kind is not v.KEYWORD_ONLY]
        assert got == want, name
        extra = {p for p, v in ps.items() if v.kind is v.KEYWORD_ONLY}
        assert extra <= {"noise", "seed", "sample0"}, name      # what this project adds is keyword-only, as on its DDIM / PLMS samplers


def test_posterior_helpers_match_the_reference_on_any_device():
    g = golden("anc_uncond")
    m = _model()
    x, e = torch.from_numpy(g["step_x"]), torch.from_numpy(g["step_e"])
    t = torch.tensor([500, 0])
    assert torch.allclose(m.predict_start_from_noise(x, t, e), torch.from_numpy(g["psfn"]), rtol=1e-6, atol=1e-6)
    assert torch.allclose(m.predict_start_from_noise(x, t, e, ch_start=3, ch_end=6), torch.from_numpy(g["psfn_ch"]), rtol=1e-6, atol=1e-6)
    qm, qv, ql = m.q_posterior(e, x, torch.tensor([999, 1]), ch_start=0, ch_end=3)
    assert torch.allclose(qm, torch.from_numpy(g["qp_mean"]), rtol=1e-6, atol=1e-6)
    assert torch.equal(qv, torch.from_numpy(g["qp_var"])) and torch.equal(ql, torch.from_numpy(g["qp_logvar"]))


def test_abi_is_8_and_the_step_descriptor_keeps_its_layout():
    assert _lib.ABI_VERSION == 8
    assert C.sizeof(_lib.STRUCTS["FridoSamplerStep"]) == 232 and C.sizeof(_lib.FridoOp) == 520      # the sizes of ABI 7
    assert _lib.OP_KINDS["FRIDO_OP_ATTN_MH"] == 26 and _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36       # the ancestral update added no kind: ABI 8's nine follow ATTN_MH
    assert _lib.OP_KINDS["FRIDO_OP_SAMPLER_STEP"] == 10
    assert _lib.STEP_ANCESTRAL not in (0, 1, 3) and _lib.STEP_ANCESTRAL & 3 == 0                    # cannot be read as a ring mode
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        assert L.frido_abi_version() == 8
        assert L.frido_sizeof_desc(_lib.OP_KINDS["FRIDO_OP_SAMPLER_STEP"]) == 232


def _step(**over):
    kw = dict(x=4096, B=2, HW=64, Cx=6, start=3, nch=3, eps_cond=8192, coef=12288, x_out=4096, pred_x0=16384, write_x=1, temperature=1.0,
              hist_mode=_lib.STEP_ANCESTRAL)
    kw.update(over)
    return _lib.make_op("FRIDO_OP_SAMPLER_STEP", **kw)[1]


@pytest.mark.parametrize("over,msg", [
    (dict(hist_ring=64, hist_stride=4096), b"no history"),
    (dict(eps_uncond=64), b"no history"),
    (dict(hist1=64), b"no history"),
    (dict(eps_out=64), b"no history"),
    (dict(HW=1, Cx=6), b"multiple of 4"),
    (dict(x=4100, x_out=4100), b"16-byte aligned"),
    (dict(pred_x0=16388), b"16-byte aligned"),
    (dict(noise=20480, noise_C=3, noise_c0=3, noise_stride=2 * 64 * 3 + 1), b"16-byte aligned"),
    (dict(noise=20480, noise_C=6, noise_c0=3), b"noise tape spans"),
    (dict(noise=20480, noise_C=2, noise_c0=4), b"noise tape spans"),
    (dict(start=4), b"bad channel range"),
    (dict(x_out=0), b"x_out missing"),
    (dict(coef=0), b"null pointer"),
])
def test_launcher_rejects_bad_ancestral_descriptors_without_touching_a_device(over, msg):
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        st = _step(**over)
        assert L.frido_sampler_step(C.addressof(st), None) == -1
        assert msg in L.frido_last_error(), L.frido_last_error()


def test_other_hist_modes_are_still_rejected_as_before():
    L = _lib.lib()
    for mode in (2, 4, 17):      # neither a ring mode nor the ancestral value
        st = _step(hist_mode=mode, hist_ring=64, hist_stride=4096, step=128)
        assert L.frido_sampler_step(C.addressof(st), None) == -1 and b"hist ring" in L.frido_last_error()


def test_refused_options_raise_with_their_name():
    m = _model()
    x, t = torch.zeros(2, 6, 16, 16), torch.zeros(2, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="quantize_denoised"):
        m.p_sample_loop(None, (2, 6, 16, 16), quantize_denoised=True)
    with pytest.raises(NotImplementedError, match="quantize_denoised"):
        m.p_sample(x, None, t, 0, quantize_denoised=True)
    with pytest.raises(NotImplementedError, match="return_codebook_ids"):
        m.p_mean_variance(x, None, t, 0, False, return_codebook_ids=True)
    with pytest.raises(NotImplementedError, match="mask / x0"):
        m.p_sample_loop(None, (2, 6, 16, 16), mask=torch.ones(2, 1, 16, 16), x0=x)
    with pytest.raises(NotImplementedError, match="mask / x0"):
        m.progressive_denoising(None, (6, 16, 16), batch_size=2, x0=x)
    with pytest.raises(NotImplementedError, match="dict conditionings"):
        m.sample(dict(c_crossattn=[x]), batch_size=2)
    ms = _model(num_timesteps_cond=2)
    with pytest.raises(NotImplementedError, match="shorten_cond_schedule"):
        ms.p_sample_loop(None, (2, 6, 16, 16))
    mn = _model(dict(AB_SMP, use_split_head=False, split_embed_dim_list=[]))
    with pytest.raises(NotImplementedError, match="use_split_head"):
        mn.p_sample_loop(None, (2, 6, 16, 16))


def test_cpu_tensors_raise_frido_hip_error():
    m = _model()
    x, t = torch.zeros(2, 6, 16, 16), torch.zeros(2, dtype=torch.long)
    with pytest.raises(_lib.FridoHipError, match="no CPU fallback"):
        m.p_sample(x, None, t, 0)
    with pytest.raises(_lib.FridoHipError, match="no CPU fallback"):
        m.p_mean_variance(x, None, t, 0, False)
    for call in (lambda: m.p_sample_loop(None, (2, 6, 16, 16), timesteps=2), lambda: m.sample(None, batch_size=2, timesteps=2),
                 lambda: m.progressive_denoising(None, (6, 16, 16), batch_size=2, start_T=2),
                 lambda: m.sample_log(None, 2, ddim=False, ddim_steps=None, timesteps=2)):
        with pytest.raises(_lib.FridoHipError, match="no CPU fallback"):
            call()
