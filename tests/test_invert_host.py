"""CPU-side checks of DDIM inversion (DDIMSampler.invert): the coefficient table against its float64 formulas, the row's exact-inverse
property, the round trip on an analytic Gaussian data model, the launcher in the header and in both builds, its argument checks (no device
is touched), its op kind in ABI 8 and every refusal of `invert` with its name."""
import ctypes as C

import numpy as np
import pytest
import torch

from golden_cfg import UNET_SMALL, VQ_SMALL, BERT_SMALL, frido_cfg
from frido_amd import _lib, patching, runtime, samplers, schedules

LINEAR = dict(linear_start=0.0015, linear_end=0.0155)      # the shipped schedule
F32_HALF_ULP = 2.0 ** -24                                   # one rounding to float32, relative
INVERSE_BOUND = 1e-12                                       # the issue's: one inversion row then the eta = 0 update of the same row, float64


def _ac32():
    return np.cumprod(1.0 - schedules.make_beta_schedule("linear", 1000, **LINEAR)).astype(np.float32)


def _grid(S):
    """(ddim_timesteps, ddim_alphas, ddim_alphas_prev) in float64, the values make_schedule(S, ddim_eta=0) leaves on the sampler."""
    ts = schedules.make_ddim_timesteps("uniform", S, 1000)
    _, al, alp = schedules.make_ddim_sampling_parameters(_ac32(), ts, 0.0)
    return ts, al.astype(np.float64), np.asarray(alp, dtype=np.float64)


def _formula(a, p):
    return np.stack((np.sqrt(a / p), np.sqrt(a) * (np.sqrt(1 / a - 1) - np.sqrt(1 / p - 1))), axis=1)


def _rel(got, want):
    return float((np.abs(got - want) / np.abs(want)).max())


def _round_trip_one_row(tab, a, p):
    """Worst relative distance, over rows and a few (x, eps), between x and the DDIM eta = 0 update (ddim.py:237-268 with sigma = 0) of
    x' = c0 x + c1 eps at the same row with the same eps, all in float64."""
    worst = 0.0
    for x, e in ((0.7, -1.3), (-0.2, 0.9), (1.0, 0.5), (-1.1, -0.4)):
        up = tab[:, 0] * x + tab[:, 1] * e
        back = np.sqrt(p) * (up - np.sqrt(1 - a) * e) / np.sqrt(a) + np.sqrt(1 - p) * e
        worst = max(worst, float((np.abs(back - x) / abs(x)).max()))
    return worst


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S, rows", [(6, 7), (50, 50), (200, 200)])
def test_table_is_the_float64_formula_rounded_once_and_inverts_the_ddim_row(S, rows):
    ts, a, p = _grid(S)
    tab = schedules.ddim_inversion_table(a.astype(np.float32), p)
    want = _formula(a, p)
    assert tab.dtype == np.float32 and tab.shape == (rows, 2) and len(ts) == rows
    assert np.array_equal(tab, want.astype(np.float32))
    err = _rel(tab.astype(np.float64), want)
    inv = _round_trip_one_row(want, a, p)
    print(f"S = {S}: table vs float64 {err:.2e} (bound {F32_HALF_ULP:.2e}); one row up and down in float64 {inv:.2e} (bound {INVERSE_BOUND:.0e})")
    assert err <= F32_HALF_ULP and inv <= INVERSE_BOUND
    assert np.all(tab[:, 0] < 1) and np.all(tab[:, 0] > 0) and np.all(tab[:, 1] > 0)      # the signal shrinks, eps is added
    # after k rows the state sits at ddim_alphas[k - 1]: the product of the c0 is sqrt(alphas[k - 1] / alphas_prev[0])
    assert np.allclose(np.cumprod(want[:, 0]), np.sqrt(a / p[0]), rtol=1e-13)


@pytest.mark.parametrize("S", [6, 50, 200])
@pytest.mark.parametrize("variant", ["swapped", "rows_plus_1", "rows_minus_1"])
def test_wrong_table_variants_miss_both_bounds_tenfold(S, variant):
    _, a, p = _grid(S)
    want = _formula(a, p)
    if variant == "swapped":
        wrong, keep = _formula(p, a), slice(None)
    elif variant == "rows_plus_1":
        wrong, keep = np.roll(want, -1, axis=0), slice(0, -1)
    else:
        wrong, keep = np.roll(want, 1, axis=0), slice(1, None)
    err = _rel(wrong[keep], want[keep])
    inv = _round_trip_one_row(wrong[keep], a[keep], p[keep])
    print(f"S = {S}, {variant}: vs the formula {err:.2e}, one row up and down {inv:.2e}")
    assert err >= 10 * F32_HALF_ULP and inv >= 10 * INVERSE_BOUND


# ---- 2. the analytic Gaussian data model ----------------------------------------------------------------------------------------------
def _gauss_round_trip(S, s2=1.0):
    """Data ~ N(0, s2), so the exact eps at level ac is eps*(x, ac) = sqrt(1 - ac) x / (ac s2 + 1 - ac) (the model tests/test_dpm_host.py
    uses for the solver's order).  Float64: k = S inversion rows up, eps at ddim_timesteps[i] -- level a, where the state is still at p --
    then DDIM eta = 0 down the same rows; returns max |x - x_start|."""
    _, a, p = _grid(S)
    assert len(a) == S
    tab = _formula(a, p)
    eps = lambda x, ac: np.sqrt(1 - ac) * x / (ac * s2 + 1 - ac)
    x0 = np.array([1.3, -0.7, 0.2])
    x = x0.copy()
    for i in range(S):
        x = tab[i, 0] * x + tab[i, 1] * eps(x, a[i])
    for i in range(S - 1, -1, -1):
        e = eps(x, a[i])
        x = np.sqrt(p[i]) * (x - np.sqrt(1 - a[i]) * e) / np.sqrt(a[i]) + np.sqrt(1 - p[i]) * e
    return float(np.abs(x - x0).max())


GAUSS_MEASURED = {10: 3.863e-02, 20: 9.837e-03, 40: 2.452e-03}      # this test's own print on the CPU


def test_round_trip_error_on_the_gaussian_model_falls_with_the_step_count():
    """Invert k = S rows, then DDIM eta = 0 back, on the shipped linear schedule in float64: the error is the discretisation
    error of evaluating eps one level above the state on the way up and at the state's own level on the way down; it falls about
    fourfold per doubling of S.  Measured here on the CPU: S = 10: 3.863e-02, S = 20: 9.837e-03, S = 40: 2.452e-03; each is asserted at 2 x that (libm differences between hosts)."""
    errs = {S: _gauss_round_trip(S) for S in (10, 20, 40)}
    print("round trip on the Gaussian model: " + ", ".join(f"S = {S}: {e:.3e}" for S, e in errs.items()))
    assert errs[10] > errs[20] > errs[40]
    for S, e in errs.items():
        assert e <= 2 * GAUSS_MEASURED[S], (S, e)


# ---- 3. the launcher and the ABI ------------------------------------------------------------------------------------------------------
def test_header_declares_the_launcher_and_its_op_kind():
    assert "frido_invert_step" in _lib.declared_symbols() and "frido_invert_step" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 8
    assert _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36 and _lib.OP_KINDS["FRIDO_OP_ATTN_MH"] == 26
    assert C.sizeof(_lib.FridoOp) == 520 and C.sizeof(_lib.STRUCTS["FridoSamplerStep"]) == 232
    assert C.sizeof(_lib.STRUCTS["FridoDpmStep"]) == 112 and C.sizeof(_lib.STRUCTS["FridoKeepBlend"]) == 120
    assert _lib.OP_KINDS["FRIDO_OP_INVERT_STEP"] == 34 and _lib.KIND_STRUCT["FRIDO_OP_INVERT_STEP"] == "FridoInvertStep"
    assert _lib.OP_KINDS["FRIDO_OP_KEEP_BLEND"] == 33 and _lib.KIND_STRUCT["FRIDO_OP_KEEP_BLEND"] == "FridoKeepBlend"
    assert C.sizeof(_lib.STRUCTS["FridoInvertStep"]) == 80


@pytest.mark.parametrize("planes", ["f16", "bf16"])
def test_both_builds_export_the_launcher_and_agree_on_the_struct_size(planes):
    L = _lib.lib(planes)
    assert hasattr(L, "frido_invert_step")
    assert L.frido_sizeof_desc(_lib.OP_KINDS["FRIDO_OP_INVERT_STEP"]) == L.frido_sizeof_desc(34) == C.sizeof(_lib.STRUCTS["FridoInvertStep"])
    assert L.frido_sizeof_desc(1002) == -1      # the kind-less descriptor code of ABI 7 is gone
    assert L.frido_abi_version() == 8


I_OK = dict(x=0x1000, eps_cond=0x2000, eps_uncond=0x3000, cfg_dev=0x4000, coef=0x5000, step=0x6000, B=3, HW=35, Cx=9, c_lo=3, c_hi=6,
            cfg_scale=1.5)


@pytest.mark.parametrize("over, msg", [
    (dict(x=None), b"null pointer"), (dict(eps_cond=None), b"null pointer"), (dict(coef=None), b"null pointer"),
    (dict(B=0), b"must be positive"), (dict(B=-1), b"must be positive"), (dict(HW=0), b"must be positive"), (dict(Cx=0), b"must be positive"),
    (dict(c_lo=-1), b"channel window"), (dict(c_lo=6), b"channel window"), (dict(c_lo=4, c_hi=4), b"channel window"),
    (dict(c_hi=10), b"channel window"), (dict(c_lo=2 ** 31 - 1), b"channel window"),
    (dict(coef_row_offset=-1), b"coef_row_offset"), (dict(cfg_scale=float("nan")), b"cfg_scale is NaN"),
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) if isinstance(o, dict) else None)
@pytest.mark.parametrize("planes", ["f16", "bf16"])
def test_invert_step_rejects_bad_descriptors_without_touching_a_device(over, msg, planes):
    L = _lib.lib(planes)
    d = _lib.STRUCTS["FridoInvertStep"](**dict(I_OK, **over))
    assert L.frido_invert_step(C.byref(d), None) == -1, over
    err = L.frido_last_error()
    assert b"frido_invert_step" in err and msg in err, err
    assert L.frido_invert_step(None, None) == -1 and b"frido_invert_step" in L.frido_last_error()


# ---- 4. the public entry point's refusals ---------------------------------------------------------------------------------------------
def _model(**over):
    from frido_amd.models import instantiate_from_config
    cfg = frido_cfg(UNET_SMALL, VQ_SMALL, BERT_SMALL)
    cfg["cond_stage_config"], cfg["cond_stage_trainable"], cfg["conditioning_key"] = "__is_unconditional__", False, "crossattn"
    cfg.update(over)
    return instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg)).eval()


@pytest.fixture(scope="module")
def model():
    return _model()


CTX, Z0 = torch.zeros(2, 5, 64), torch.zeros(2, 6, 16, 16)


def _invert(sampler, cond=CTX, z0=Z0, **kw):
    kw = dict(dict(t_start=3, num_stage=2, verbose=False), **kw)
    return sampler.invert(6, z0, cond, **kw)


@pytest.mark.parametrize("name", ["PLMSSampler", "DPMSolverSampler"])
def test_the_other_samplers_refuse_invert_by_name(model, name):
    with pytest.raises(NotImplementedError, match=name):
        _invert(getattr(samplers, name)(model))


@pytest.mark.parametrize("kw, word", [
    (dict(score_corrector=object()), "score_corrector"),
    (dict(cond=dict(c_crossattn=[CTX])), "dict / list conditioning"), (dict(cond=[CTX]), "dict / list conditioning"),
    (dict(unconditional_conditioning=[CTX], unconditional_guidance_scale=2.0), "dict / list conditioning"),
])
def test_what_invert_cannot_honour_is_refused_by_name(model, kw, word):
    with pytest.raises(NotImplementedError, match=word):
        _invert(samplers.DDIMSampler(model), **kw)


def test_split_input_params_is_refused():
    m = _model()
    m.split_input_params = dict(ks=(8, 8), stride=(4, 4))
    with pytest.raises(NotImplementedError, match="split_input_params"):
        _invert(samplers.DDIMSampler(m))


@pytest.mark.parametrize("kw, word", [
    (dict(t_start=0), "t_start"), (dict(t_start=7), "t_start"), (dict(t_start=2.0), "t_start"), (dict(t_start=None), "exactly one"),
    (dict(strength=0.5), "exactly one"),
    (dict(first_stage=2), "first_stage"), (dict(first_stage=-1), "first_stage"), (dict(num_stage=1, first_stage=1), "first_stage"),
    (dict(z0=torch.zeros(6, 16, 16)), "latent to invert"), (dict(z0=None), "latent to invert"),
])
def test_bad_invert_arguments_are_value_errors(model, kw, word):
    with pytest.raises(ValueError, match=word):
        _invert(samplers.DDIMSampler(model), **kw)


def test_cpu_tensors_raise_the_hip_error(model):
    with pytest.raises(_lib.FridoHipError, match="no CPU path"):
        _invert(samplers.DDIMSampler(model))
    with pytest.raises(_lib.FridoHipError, match="no CPU path"):
        samplers.DDIMSampler(model).invert(6, Z0, CTX, strength=0.5, num_stage=2, verbose=False)


def test_encode_is_inverts_alias_in_upstreams_argument_order(model):
    s = samplers.DDIMSampler(model)
    with pytest.raises(NotImplementedError, match="make_schedule"):
        s.encode(Z0, CTX, 3)
    s.make_schedule(6, verbose=False)
    with pytest.raises(ValueError, match="t_start"):
        s.encode(Z0, CTX, 7, num_stage=2, verbose=False)
    with pytest.raises(_lib.FridoHipError, match="no CPU path"):
        s.encode(Z0, CTX, 3, num_stage=2, verbose=False)


def test_the_engine_kind_lays_its_tables_out_in_ascending_order():
    """The inversion kind's cache key is its own, and its timestep / coefficient rows ascend (read without a device: the table code only)."""
    ts, a, p = _grid(6)
    assert np.all(np.diff(ts) > 0) and ts[0] == 1
    tab, t_desc = schedules.sampler_coef_table(_ac32(), 6, 0.0)
    assert np.array_equal(t_desc[::-1], ts)      # DDIM's loop order is the same grid, descending
    inv = schedules.ddim_inversion_table(a, p)
    # row i of the inversion undoes DDIM's loop row n - 1 - i: same (a_t, a_prev)
    assert np.array_equal(tab[::-1, 0], a.astype(np.float32)) and np.array_equal(tab[::-1, 1], p.astype(np.float32)) and inv.shape[0] == tab.shape[0]
