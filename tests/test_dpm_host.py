"""CPU-side checks of the DPM-Solver++(2M) sampler: the coefficient table's identities in float64, the solver's order of convergence on an
analytic Gaussian data model (a float64 loop of the test's own over the table), the logSNR grid, every refusal with its name, the
launcher in the header and in both builds, its argument checks (no device is touched) and its op kind in ABI 8."""
import ctypes as C

import numpy as np
import pytest
import torch

from golden_cfg import UNET_SMALL, VQ_SMALL, BERT_SMALL, frido_cfg
from frido_amd import _lib, schedules

LINEAR = dict(linear_start=0.0015, linear_end=0.0155)      # the shipped schedule


def _ac():
    return np.cumprod(1.0 - schedules.make_beta_schedule("linear", 1000, **LINEAR))


# ---- 1. table identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 50, 200])
def test_first_order_rows_on_the_uniform_grid_are_the_ddim_eta0_step(S):
    """c_x x + c_d x0 = sqrt(ac_next) x0 + sqrt(1 - ac_next) e for x = alpha x0 + sigma e, in float64 before the table is rounded."""
    ac32 = _ac().astype(np.float32)
    t_loop, cur, nxt = schedules.dpm_solver_grid(ac32, S, "time_uniform")
    rows = schedules.dpm_solver_rows(cur, nxt, order=1)
    ts = schedules.make_ddim_timesteps("uniform", S, 1000)
    _, al, alp = schedules.make_ddim_sampling_parameters(ac32, ts, 0.0)
    assert np.array_equal(t_loop, ts[::-1]) and np.array_equal(cur, al[::-1].astype(np.float64)) and np.array_equal(nxt, alp[::-1])
    assert rows.dtype == np.float64 and rows.shape == (len(ts), schedules.DPM_ROW)
    assert np.array_equal(rows[:, 4:], np.tile([1.0, 0, 0, 0], (len(ts), 1)))
    worst = 0.0
    for x0, e in ((0.7, -1.3), (-0.2, 0.9), (1.0, 0.0), (0.0, 1.0)):
        x = np.sqrt(cur) * x0 + np.sqrt(1 - cur) * e
        got = rows[:, 2] * x + rows[:, 3] * x0
        want = np.sqrt(nxt) * x0 + np.sqrt(1 - nxt) * e
        worst = max(worst, float((np.abs(got - want) / np.abs(want)).max()))
        assert np.allclose((x - rows[:, 1] * e) * rows[:, 0], x0, rtol=1e-12, atol=1e-15)      # inv_alpha, sigma recover x0
    print(f"S = {S}: worst relative deviation from the DDIM eta = 0 step {worst:.2e}")
    assert worst <= 1e-12
    t2, tab = schedules.dpm_solver_table(ac32, S, "time_uniform", 1, True)
    assert tab.dtype == np.float32 and np.array_equal(tab, rows.astype(np.float32)) and np.array_equal(t2, t_loop)


# ---- 2. order of convergence --------------------------------------------------------------------------------------------------------
def _end_error(ac, s2, S, skip_type, order):
    """Float64 loop over the (unrounded) table on the analytic model: data ~ N(0, s2), so eps*(x, t) = sigma_t x / (ac_t s2 + 1 - ac_t) and
    the probability-flow ODE carries x_T to x_T sqrt((ac_0 s2 + 1 - ac_0) / (ac_{T-1} s2 + 1 - ac_{T-1})) exactly."""
    t_loop, cur, nxt = schedules.dpm_solver_grid(ac, S, skip_type)
    rows = schedules.dpm_solver_rows(cur, nxt, order=order, lower_order_final=True)
    x_T = np.array([1.3, -0.7, 0.2])
    x, hist = x_T.copy(), np.zeros(3)
    for i in range(len(t_loop)):
        inv_alpha, sigma, c_x, c_d, w_cur, w_last = rows[i, :6]
        e = sigma * x / (cur[i] * s2 + 1.0 - cur[i])
        x0 = (x - sigma * e) * inv_alpha
        D = x0 if w_last == 0 else w_cur * x0 + w_last * hist
        x, hist = c_x * x + c_d * D, x0
    var = lambda a: a * s2 + 1.0 - a
    exact = x_T * np.sqrt(var(nxt[-1]) / var(cur[0]))
    return float(np.abs(x - exact).max())


@pytest.mark.parametrize("s2", [0.25, 1.0, 4.0])
def test_second_order_convergence_on_the_logsnr_grid(s2):
    ac = _ac()
    e20, e40 = _end_error(ac, s2, 20, "logSNR", 2), _end_error(ac, s2, 40, "logSNR", 2)
    print(f"s^2 = {s2}: err(2M, logSNR, 20) = {e20:.3e}, err(2M, logSNR, 40) = {e40:.3e}, ratio {e20 / e40:.2f}")
    assert e20 / e40 >= 3


@pytest.mark.parametrize("s2", [0.25, 1.0])
def test_twenty_second_order_steps_beat_two_hundred_ddim_steps(s2):
    ac = _ac()
    e2m, eddim = _end_error(ac, s2, 20, "logSNR", 2), _end_error(ac.astype(np.float32), s2, 200, "time_uniform", 1)
    print(f"s^2 = {s2}: err(2M, logSNR, 20) = {e2m:.3e}, err(DDIM eta 0, uniform, 200) = {eddim:.3e}")
    assert e2m < eddim


# ---- 3. grid ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 6, 20, 40, 200, 1500])
def test_logsnr_grid_runs_from_the_last_timestep_to_zero(S):
    ac = _ac()
    t_loop, cur, nxt = schedules.dpm_solver_grid(ac, S, "logSNR")
    n = len(t_loop)
    assert 1 <= n <= S and t_loop[0] == 999 and np.all(np.diff(t_loop) < 0) and t_loop.dtype == np.int64
    assert np.array_equal(cur, ac[t_loop]) and np.array_equal(nxt[:-1], ac[t_loop[1:]]) and nxt[-1] == ac[0]      # ... > t_n = 0
    # every grid point is the timestep nearest to its uniform-in-lambda target
    lam = 0.5 * np.log(ac / (1 - ac))
    v = lam[999] + np.arange(S + 1) * (lam[0] - lam[999]) / S
    want = sorted({int(np.abs(lam - x).argmin()) for x in v}, reverse=True)
    assert want[0] == 999 and want[-1] == 0 and list(t_loop) == want[:-1]


def test_forty_steps_collapse_to_thirty_nine_on_the_shipped_schedule():
    t_loop, tab = schedules.dpm_solver_table(_ac(), 40)
    assert len(t_loop) == 39 and tab.shape == (39, 8) and tab.dtype == np.float32


@pytest.mark.parametrize("skip_type", ["logSNR", "time_uniform"])
def test_first_and_last_rows_are_first_order(skip_type):
    ac = _ac()
    for lof in (True, False):
        _, tab = schedules.dpm_solver_table(ac, 20, skip_type, 2, lof)
        assert tab[0, 4] == 1 and tab[0, 5] == 0                      # the first row of every stage: the table is walked from its top
        assert np.all(tab[1:-1, 5] < 0) and np.allclose(tab[1:-1, 4] + tab[1:-1, 5], 1.0, atol=1e-6)
        assert (tab[-1, 4] == 1 and tab[-1, 5] == 0) if lof else tab[-1, 5] < 0
        assert np.all(tab[:, 6:] == 0) and np.all(np.isfinite(tab))
    _, tab1 = schedules.dpm_solver_table(ac, 20, skip_type, 1, True)
    assert np.all(tab1[:, 4] == 1) and np.all(tab1[:, 5] == 0)
    # second-order weights: w_cur = 1 + 1 / 2r, w_last = -1 / 2r with r = h_prev / h, from the grid's own lambdas
    t_loop, cur, nxt = schedules.dpm_solver_grid(ac, 20, skip_type)
    lam = lambda a: 0.5 * np.log(a / (1 - a))
    h = lam(nxt) - lam(cur)
    rows = schedules.dpm_solver_rows(cur, nxt, 2, False)
    assert np.allclose(rows[1:, 5], -h[1:] / (2 * h[:-1]), rtol=1e-12) and np.allclose(rows[1:, 4], 1 + h[1:] / (2 * h[:-1]), rtol=1e-12)


def test_schedule_refusals():
    ac = _ac()
    with pytest.raises(ValueError, match="order"):
        schedules.dpm_solver_table(ac, 20, "logSNR", 3, True)
    with pytest.raises(ValueError, match="skip_type"):
        schedules.dpm_solver_table(ac, 20, "quad", 2, True)
    with pytest.raises(ValueError, match="no step"):
        schedules.dpm_solver_table(ac[:1], 20)
    with pytest.raises(ValueError):
        schedules.dpm_solver_table(ac, 0)


# ---- 4. refusals and the ABI --------------------------------------------------------------------------------------------------------
def _model(**over):
    from frido_amd.models import instantiate_from_config
    cfg = frido_cfg(UNET_SMALL, VQ_SMALL, BERT_SMALL)
    cfg["cond_stage_config"], cfg["cond_stage_trainable"], cfg["conditioning_key"] = "__is_unconditional__", False, "crossattn"
    cfg.update(over)
    return instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg)).eval()


@pytest.fixture(scope="module")
def sampler():
    from frido.models.diffusion.dpm_solver import DPMSolverSampler
    from frido_amd import samplers
    assert DPMSolverSampler is samplers.DPMSolverSampler and DPMSolverSampler.KIND == "dpm"
    return DPMSolverSampler(_model())


CTX = torch.zeros(2, 5, 64)


def _sample(s, cond=CTX, **kw):
    return s.sample(S=6, batch_size=2, shape=(6, 16, 16), conditioning=cond, num_stage=2, verbose=False, **kw)


@pytest.mark.parametrize("kw, word", [
    (dict(eta=1.0), "eta"), (dict(temperature=0.5), "temperature"), (dict(noise_dropout=0.1), "noise_dropout"),
    (dict(score_corrector=object()), "score_corrector"), (dict(mask=torch.ones(2, 1, 16, 16)), "mask / x0"), (dict(x0=torch.zeros(2, 6, 16, 16)), "mask / x0"),
    (dict(quantize_x0=True), "quantize_x0"),
])
def test_options_the_solver_cannot_honour_are_refused_by_name(sampler, kw, word):
    with pytest.raises(NotImplementedError, match=word):
        _sample(sampler, **kw)


@pytest.mark.parametrize("cond", [dict(c_crossattn=[CTX]), [CTX]], ids=["dict", "list"])
def test_dict_and_list_conditionings_are_refused(sampler, cond):
    with pytest.raises(NotImplementedError, match="dict / list conditionings"):
        _sample(sampler, cond=cond)
    with pytest.raises(NotImplementedError, match="dict / list conditionings"):
        _sample(sampler, unconditional_conditioning=cond, unconditional_guidance_scale=2.0)


def test_split_input_params_is_refused_in_the_patch_modes_wording():
    from frido_amd import patching
    from frido_amd.samplers import DPMSolverSampler
    m = _model()
    m.split_input_params = dict(ks=(8, 8), stride=(4, 4))
    with pytest.raises(NotImplementedError, match="split_input_params") as ei:
        _sample(DPMSolverSampler(m))
    assert str(ei.value) == str(patching.refuse("DPMSolverSampler"))


def test_bad_solver_options_are_value_errors(sampler):
    for order in (0, 3, "2"):
        with pytest.raises(ValueError, match="order"):
            _sample(sampler, order=order)
    with pytest.raises(ValueError, match="skip_type"):
        _sample(sampler, skip_type="quad")


def test_a_one_timestep_model_has_no_step_to_take():
    from frido_amd.samplers import DPMSolverSampler
    m = _model()
    m.alphas_cumprod = m.alphas_cumprod[:1]
    with pytest.raises(ValueError, match="no step"):
        _sample(DPMSolverSampler(m))


def test_cpu_conditioning_raises_the_hip_error(sampler):
    with pytest.raises(_lib.FridoHipError, match="no CPU path"):
        _sample(sampler)


def test_pipeline_refuses_an_eta_for_the_solver():
    from frido_amd.pipeline import sample_images
    with pytest.raises(ValueError, match="eta"):
        sample_images(_model(), CTX, S=6, sampler="dpm", eta=0.5)


def test_header_declares_the_launcher_and_its_op_kind():
    assert "frido_dpm_step" in _lib.declared_symbols() and "frido_dpm_step" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 8
    assert _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36 and _lib.OP_KINDS["FRIDO_OP_ATTN_MH"] == 26
    assert C.sizeof(_lib.FridoOp) == 520 and C.sizeof(_lib.STRUCTS["FridoGemm"]) == 512
    assert C.sizeof(_lib.STRUCTS["FridoSamplerStep"]) == 232
    assert _lib.OP_KINDS["FRIDO_OP_DPM_STEP"] == 32 and _lib.KIND_STRUCT["FRIDO_OP_DPM_STEP"] == "FridoDpmStep"
    assert C.sizeof(_lib.STRUCTS["FridoDpmStep"]) == 112
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        assert L.frido_abi_version() == 8
        assert L.frido_sizeof_desc(32) == C.sizeof(_lib.STRUCTS["FridoDpmStep"]) and hasattr(L, "frido_dpm_step")


def test_both_builds_export_the_launcher():
    for planes in ("f16", "bf16"):
        assert hasattr(_lib.lib(planes), "frido_dpm_step"), planes


D_OK = dict(x=0x1000, B=2, HW=15, Cx=6, start=3, nch=3, eps_cond=0x2000, eps_uncond=0x3000, cfg_scale=1.5, coef=0x4000, step=0x5000,
            x_out=0x1000, pred_x0=0x6000, x0_hist=0x7000)


@pytest.mark.parametrize("over", [
    dict(x=None), dict(eps_cond=None), dict(coef=None), dict(x_out=None), dict(x0_hist=None), dict(B=0), dict(B=-1), dict(HW=0), dict(Cx=0),
    dict(nch=0), dict(start=-1), dict(start=4), dict(start=0, nch=7), dict(start=2 ** 31 - 1, nch=3), dict(cfg_scale=float("nan")),
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
@pytest.mark.parametrize("planes", ["f16", "bf16"])
def test_dpm_step_rejects_bad_descriptors_without_touching_a_device(over, planes):
    L = _lib.lib(planes)
    d = _lib.STRUCTS["FridoDpmStep"](**dict(D_OK, **over))
    assert L.frido_dpm_step(C.byref(d), None) == -1, over
    assert b"frido_dpm_step" in L.frido_last_error()
    assert L.frido_dpm_step(None, None) == -1 and b"frido_dpm_step" in L.frido_last_error()
