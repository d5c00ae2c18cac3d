"""CPU-side checks of composed guidance (compose= / guidance_rescale=): the launcher in the header and in both builds, its argument checks
(no device is touched), its op kind in ABI 8, every ValueError and by-name refusal of the public keywords, the engine-cache key of a
call without them, and the arithmetic on an analytic equal-variance Gaussian family in float64."""
import ctypes as C

import numpy as np
import pytest
import torch

from golden_cfg import UNET_SMALL, VQ_SMALL, BERT_SMALL, frido_cfg
from frido_amd import _lib, patching, runtime, samplers, schedules

LINEAR = dict(linear_start=0.0015, linear_end=0.0155)      # the shipped schedule


# ---- 1. the launcher and the ABI ------------------------------------------------------------------------------------------------------
def test_header_declares_the_launcher_and_its_op_kind():
    assert "frido_guidance_compose" in _lib.declared_symbols() and "frido_guidance_compose" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 8
    assert _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36 and _lib.OP_KINDS["FRIDO_OP_ATTN_MH"] == 26
    assert C.sizeof(_lib.FridoOp) == 520 and C.sizeof(_lib.STRUCTS["FridoSamplerStep"]) == 232
    assert C.sizeof(_lib.STRUCTS["FridoDpmStep"]) == 112 and C.sizeof(_lib.STRUCTS["FridoKeepBlend"]) == 120
    assert C.sizeof(_lib.STRUCTS["FridoInvertStep"]) == 80
    assert _lib.OP_KINDS["FRIDO_OP_GUIDANCE_COMPOSE"] == 35 and _lib.KIND_STRUCT["FRIDO_OP_GUIDANCE_COMPOSE"] == "FridoGuidanceCompose"
    assert _lib.OP_KINDS["FRIDO_OP_INVERT_STEP"] == 34 and _lib.KIND_STRUCT["FRIDO_OP_INVERT_STEP"] == "FridoInvertStep"
    assert _lib.OP_KINDS["FRIDO_OP_KEEP_BLEND"] == 33 and _lib.KIND_STRUCT["FRIDO_OP_KEEP_BLEND"] == "FridoKeepBlend"
    assert C.sizeof(_lib.STRUCTS["FridoGuidanceCompose"]) == 40
    assert runtime.GUIDANCE_MAX == samplers.COMPOSE_MAX + 1 == 8


@pytest.mark.parametrize("planes", ["f16", "bf16"])
def test_both_builds_export_the_launcher_and_agree_on_the_struct_size(planes):
    L = _lib.lib(planes)
    assert hasattr(L, "frido_guidance_compose")
    assert L.frido_sizeof_desc(_lib.OP_KINDS["FRIDO_OP_GUIDANCE_COMPOSE"]) == L.frido_sizeof_desc(35) == C.sizeof(_lib.STRUCTS["FridoGuidanceCompose"])
    assert L.frido_sizeof_desc(1003) == -1      # the kind-less descriptor code of ABI 7 is gone
    assert L.frido_abi_version() == 8


EPS, TOTAL = 0x100000, 3 * 105 * 4        # slot 0's address; bytes per slot of G_OK
G_OK = dict(eps=EPS, out=EPS, weights=0x5000, n=3, B=3, per_sample=105, rescale=0)


@pytest.mark.parametrize("over, msg", [
    (dict(eps=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(weights=None), b"null pointer"),
    (dict(n=0), b"1 to 8 conditionings"), (dict(n=9), b"1 to 8 conditionings"), (dict(n=-1), b"1 to 8 conditionings"),
    (dict(B=0), b"must be positive"), (dict(B=-1), b"must be positive"), (dict(per_sample=0), b"must be positive"),
    (dict(per_sample=-5), b"must be positive"),
    (dict(out=EPS + TOTAL), b"must not overlap"), (dict(out=EPS + 2 * TOTAL), b"must not overlap"),         # slots 1 and 2
    (dict(out=EPS + 3 * TOTAL), b"must not overlap"),                                                        # the unconditional slot
    (dict(out=EPS + 4 * TOTAL - 4), b"must not overlap"), (dict(out=EPS + 4), b"must not overlap"),          # partly inside
    (dict(out=EPS - 4), b"must not overlap"),                                                                # slot 0, but not exactly
    (dict(out=EPS + TOTAL, rescale=1), b"must not overlap"),
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) if isinstance(o, dict) else None)
@pytest.mark.parametrize("planes", ["f16", "bf16"])
def test_guidance_compose_rejects_bad_descriptors_without_touching_a_device(over, msg, planes):
    L = _lib.lib(planes)
    d = _lib.STRUCTS["FridoGuidanceCompose"](**dict(G_OK, **over))
    assert L.frido_guidance_compose(C.byref(d), None) == -1, over
    err = L.frido_last_error()
    assert b"frido_guidance_compose" in err and msg in err, err
    assert L.frido_guidance_compose(None, None) == -1 and b"frido_guidance_compose" in L.frido_last_error()


# ---- 2. the public keywords' refusals -------------------------------------------------------------------------------------------------
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
CALLS = ["ddim", "plms", "dpm", "edit"]


def _call(model, which, **kw):
    """The public call `which` with a composition; nothing here reaches a device: every refusal comes first."""
    kw = dict(dict(unconditional_conditioning=CTX, unconditional_guidance_scale=1.5, compose=[(CTX, 0.5)], num_stage=2, verbose=False), **kw)
    cond = kw.pop("conditioning", CTX)
    if which == "edit":
        return samplers.DDIMSampler(model).edit(6, Z0, cond, t_start=3, **kw)
    cls = dict(ddim=samplers.DDIMSampler, plms=samplers.PLMSSampler, dpm=samplers.DPMSolverSampler)[which]
    return cls(model).sample(S=6, batch_size=2, shape=(6, 16, 16), conditioning=cond, **kw)


@pytest.mark.parametrize("which", CALLS)
@pytest.mark.parametrize("kw, word", [
    (dict(compose=[(torch.zeros(2, 4, 64), 0.5)]), r"compose\[0\] must be a tensor like conditioning"),                 # shape
    (dict(compose=[(CTX, 0.5), (torch.zeros(2, 5, 64, dtype=torch.int64), 0.5)]), r"compose\[1\] must be a tensor like"),   # dtype class
    (dict(compose=[(torch.zeros(2, 5, 64, device="meta"), 0.5)]), r"compose\[0\] must be a tensor like conditioning"),    # device
    (dict(compose=[(None, 0.5)]), r"compose\[0\] must be a tensor like conditioning"),
    (dict(compose=[(CTX, float("nan"))]), "finite real number"), (dict(compose=[(CTX, float("inf"))]), "finite real number"),
    (dict(compose=[(CTX, "2")]), "finite real number"), (dict(compose=[(CTX, 1j)]), "finite real number"),
    (dict(compose=[(CTX, True)]), "finite real number"),
    (dict(unconditional_guidance_scale=float("nan")), "finite real number"),
    (dict(compose=[(CTX, 0.1)] * 8), "at most 7"),
    (dict(guidance_rescale=-0.1), "guidance_rescale"), (dict(guidance_rescale=1.5), "guidance_rescale"),
    (dict(guidance_rescale=float("nan")), "guidance_rescale"), (dict(compose=None, guidance_rescale="0.5"), "guidance_rescale"),
    (dict(unconditional_conditioning=None), "unconditional_conditioning"),
    (dict(unconditional_conditioning=None, compose=None, guidance_rescale=0.5, unconditional_guidance_scale=1.0), "unconditional_conditioning"),
    (dict(compose=[CTX]), r"\(conditioning, weight\) pairs"),
])
def test_bad_compose_arguments_are_value_errors(model, which, kw, word):
    with pytest.raises(ValueError, match=word):
        _call(model, which, **kw)


@pytest.mark.parametrize("which", CALLS)
@pytest.mark.parametrize("kw, word", [
    (dict(compose=[(dict(c_crossattn=[CTX]), 0.5)]), "dict / list conditioning"), (dict(compose=[([CTX], 0.5)]), "dict / list conditioning"),
    (dict(compose=[(CTX, 0.5), ([CTX], 0.5)]), "dict / list conditioning"),
])
def test_dict_and_list_conditionings_inside_compose_are_refused_by_name(model, which, kw, word):
    with pytest.raises(NotImplementedError, match=word):
        _call(model, which, **kw)


@pytest.mark.parametrize("which", ["ddim", "plms"])
@pytest.mark.parametrize("kw", [dict(), dict(compose=None, guidance_rescale=0.5)], ids=["compose", "rescale"])
def test_score_corrector_with_either_keyword_is_refused_by_name(model, which, kw):
    with pytest.raises(NotImplementedError, match="score_corrector is not built for composed guidance"):
        _call(model, which, score_corrector=object(), **kw)


@pytest.mark.parametrize("which", CALLS)
@pytest.mark.parametrize("kw", [dict(), dict(compose=None, guidance_rescale=0.5)], ids=["compose", "rescale"])
def test_split_input_params_is_refused(which, kw):
    m = _model()
    m.split_input_params = dict(ks=(8, 8), stride=(4, 4))
    with pytest.raises(NotImplementedError, match="split_input_params"):
        _call(m, which, **kw)


@pytest.mark.parametrize("kw", [dict(compose=[(CTX, 0.5)]), dict(guidance_rescale=0.5)], ids=["compose", "rescale"])
def test_invert_and_encode_refuse_either_keyword_by_name(model, kw):
    s = samplers.DDIMSampler(model)
    with pytest.raises(NotImplementedError, match=r"DDIMSampler.invert: composed guidance \(compose= / guidance_rescale=\)"):
        s.invert(6, Z0, CTX, t_start=3, num_stage=2, verbose=False, unconditional_conditioning=CTX, **kw)
    s.make_schedule(6, verbose=False)
    with pytest.raises(NotImplementedError, match="composed guidance"):
        s.encode(Z0, CTX, 3, num_stage=2, verbose=False, unconditional_conditioning=CTX, **kw)


def test_the_ancestral_pipeline_route_refuses_the_keywords(model):
    from frido_amd.pipeline import sample_images
    with pytest.raises(ValueError, match="ancestral loop has no classifier-free guidance"):
        sample_images(model, CTX, S=4, sampler="ddpm", compose=[(CTX, 0.5)])
    with pytest.raises(ValueError, match="ancestral loop has no classifier-free guidance"):
        sample_images(model, CTX, S=4, sampler="ddpm", guidance_rescale=0.5)


def test_a_valid_composition_gets_as_far_as_the_device_check(model):
    """Nothing above is refused for a well-formed call: it fails only where every CPU call fails."""
    for which in CALLS:
        with pytest.raises(_lib.FridoHipError, match="no CPU path"):
            _call(model, which, compose=[(CTX, -0.75), (CTX, 0.5)], guidance_rescale=0.7)


# ---- 3. the engine-cache key ----------------------------------------------------------------------------------------------------------
def test_a_call_without_the_keywords_builds_the_key_it_always_built(model):
    s = samplers.DDIMSampler(model)
    assert s._engine_key(2, (6, 16, 16), 5, 6, 0.0, 1.5, 2, 1.0) == ("ddim", 2, 6, 16, 16, 5, 6, 0.0, True, 2, 1.0, 0)
    assert s._engine_key(2, (6, 16, 16), 5, 6, 1.0, 1.0, 2, 0.5, replica=1) == ("ddim", 2, 6, 16, 16, 5, 6, 1.0, False, 2, 0.5, 1)
    assert s._engine_key(2, (6, 16, 16), 5, 6, 0.0, 1.5, 2, 1.0, kind="invert") == ("invert", 2, 6, 16, 16, 5, 6, 0.0, True, 2, 1.0, 0)
    assert samplers.PLMSSampler(model)._engine_key(2, (6, 16, 16), "labels", 6, 0.0, 1.0, 2, 1.0) == \
        ("plms", 2, 6, 16, 16, "labels", 6, 0.0, False, 2, 1.0, 0)
    d = samplers.DPMSolverSampler(model)
    assert d._engine_key(2, (6, 16, 16), 5, 6, 0.0, 1.5, 2, 1.0, solver=(2, "logSNR", True)) == \
        ("dpm", 2, 6, 16, 16, 5, 6, True, 2, 0, 2, "logSNR", True)
    # composed: the old key with guidance on (the scale is a weight) plus one entry; neither the weights nor phi are in it
    assert s._engine_key(2, (6, 16, 16), 5, 6, 0.0, 1.0, 2, 1.0, composed=(3, True)) == \
        ("ddim", 2, 6, 16, 16, 5, 6, 0.0, True, 2, 1.0, 0, ("compose", 3, True))
    assert d._engine_key(2, (6, 16, 16), 5, 6, 0.0, 1.5, 2, 1.0, solver=(2, "logSNR", True), composed=(2, False)) == \
        ("dpm", 2, 6, 16, 16, 5, 6, True, 2, 0, 2, "logSNR", True, ("compose", 2, False))


def test_check_compose_orders_the_terms_and_leaves_a_plain_call_alone(model):
    who = "DDIMSampler.sample"
    assert samplers.check_compose(who, model, CTX, None, 1.0, None, 0.0) is None
    assert samplers.check_compose(who, model, CTX, CTX, 2.0, None, 0) is None
    assert samplers.check_compose(who, model, CTX, CTX, 2.0, [], 0.0) is None       # an empty composition without rescale is plain guidance
    c1, c2 = CTX + 1, CTX + 2
    conds, w, phi = samplers.check_compose(who, model, CTX, CTX, 1.5, [(c1, -0.75), (c2, np.float32(0.5))], 0.7)
    assert [c.data_ptr() for c in conds] == [CTX.data_ptr(), c1.data_ptr(), c2.data_ptr()] and w == [1.5, -0.75, 0.5] and phi == 0.7
    conds, w, phi = samplers.check_compose(who, model, CTX, CTX, 1.0, None, 1)
    assert len(conds) == 1 and w == [1.0] and phi == 1.0
    assert samplers._composed_call((conds, w, phi), CTX)[1:] == ((1, True), dict(weights=[1.0], phi=1.0))
    assert samplers._composed_call(None, CTX) == (CTX, None, {})


# ---- 4. the arithmetic on an equal-variance Gaussian family, float64 --------------------------------------------------------------------
def _grid(S):
    ac = np.cumprod(1.0 - schedules.make_beta_schedule("linear", 1000, **LINEAR)).astype(np.float32)
    ts = schedules.make_ddim_timesteps("uniform", S, 1000)
    _, al, alp = schedules.make_ddim_sampling_parameters(ac, ts, 0.0)
    return al.astype(np.float64), np.asarray(alp, dtype=np.float64)


def _eps_gauss(x, ac, mu, s2):
    """E[eps | x_t = x] for data ~ N(mu, s2 I) at level ac."""
    return np.sqrt(1 - ac) * (x - np.sqrt(ac) * mu) / (ac * s2 + 1 - ac)


def _compose(eps, eu, w):
    """Section 1 of the feature restated: acc = e_u; acc += w_i (e_i - e_u) in order."""
    acc = eu.copy()
    for e, wi in zip(eps, w):
        acc = acc + wi * (e - eu)
    return acc


def _ddim_down(x, a, p, eps_of):
    """The eta = 0 DDIM chain (ddim.py:237-268 with sigma = 0) over all rows, last row first."""
    for i in range(len(a) - 1, -1, -1):
        e = eps_of(x, a[i])
        x = np.sqrt(p[i]) * (x - np.sqrt(1 - a[i]) * e) / np.sqrt(a[i]) + np.sqrt(1 - p[i]) * e
    return x


def _ode_exact(x_T, a_T, a_0, mu, s2):
    """Where the probability-flow ODE of N(mu, s2 I) data carries x_T from level a_T to level a_0: the marginals are Gaussian, the flow
    keeps the standardised coordinate."""
    return np.sqrt(a_0) * mu + (x_T - np.sqrt(a_T) * mu) * np.sqrt((a_0 * s2 + 1 - a_0) / (a_T * s2 + 1 - a_T))


MU_U = np.array([0.3, -0.2, 0.1, 0.0])
MUS = [np.array([1.0, 0.5, -0.4, 0.8]), np.array([-0.6, 0.9, 0.7, -0.3]), np.array([0.2, -1.1, 0.4, 0.5])]
FAMILY_CASES = {"one": [1.5], "and": [1.0, 1.0], "negation": [1.5, -0.75], "three_mixed": [1.5, -0.75, 0.5], "zero_weight": [2.0, 0.0, 3.0]}


@pytest.mark.parametrize("S", [10, 40])
@pytest.mark.parametrize("case", sorted(FAMILY_CASES))
def test_composed_eps_is_the_eps_of_the_shifted_gaussian_and_the_chain_ends_at_its_mean(case, S):
    w = FAMILY_CASES[case]
    mus, s2 = MUS[:len(w)], 0.05 ** 2
    target = MU_U + sum(wi * (m - MU_U) for wi, m in zip(w, mus))
    a, p = _grid(S)
    x_T = np.array([0.9, -1.4, 0.3, 2.1])
    # at every noise level the composed eps IS the eps of N(target, s2 I): the family's eps is affine in the mean
    for ac in list(a) + [0.5, 0.999]:
        got = _compose([_eps_gauss(x_T, ac, m, s2) for m in mus], _eps_gauss(x_T, ac, MU_U, s2), w)
        want = _eps_gauss(x_T, ac, target, s2)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (ac, got, want)
    composed = lambda x, ac: _compose([_eps_gauss(x, ac, m, s2) for m in mus], _eps_gauss(x, ac, MU_U, s2), w)
    end = _ddim_down(x_T.copy(), a, p, composed)
    single = _ddim_down(x_T.copy(), a, p, lambda x, ac: _eps_gauss(x, ac, target, s2))
    exact = _ode_exact(x_T, a[-1], p[0], target, s2)
    disc = float(np.abs(single - exact).max())          # the chain's own discretisation error at this step count, single Gaussian
    err = float(np.abs(end - exact).max())
    spread = float(np.abs(exact - np.sqrt(p[0]) * target).max())      # the ODE's end point lies within the data's own sigma of the mean
    print(f"{case} S = {S}: composed chain vs the ODE's end {err:.3e}, single Gaussian {disc:.3e}; |end - mean| {np.abs(end - target).max():.3e} "
          f"(ODE end vs mean {spread:.3e})")
    assert err <= disc * (1 + 1e-9) + 1e-12
    assert float(np.abs(end - target).max()) <= disc + spread + (1 - np.sqrt(p[0])) * np.abs(target).max() + 1e-12
    # wrong compositions end elsewhere: by at least 10 x that error
    wrong = []
    if len(w) > 1:
        if w[0] != w[1]:
            wrong.append([w[1], w[0]] + w[2:])
        if w[-1] != 0:
            wrong.append(w[:-1] + [0.0])
    ends = [_ddim_down(x_T.copy(), a, p, lambda x, ac: _compose([_eps_gauss(x, ac, m, s2) for m in mus], _eps_gauss(x, ac, MU_U, s2), ww))
            for ww in wrong]
    # ... and so does slot 0 taken as the unconditional one
    ends.append(_ddim_down(x_T.copy(), a, p, lambda x, ac: _compose([_eps_gauss(x, ac, m, s2) for m in [MU_U] + mus[1:]],
                                                                     _eps_gauss(x, ac, mus[0], s2), w)))
    for bad in ends:
        assert float(np.abs(bad - exact).max()) >= 10 * max(disc, 1e-12), (bad, exact)


def test_the_discretisation_error_of_the_family_falls_with_the_step_count():
    a10, p10 = _grid(10)
    a40, p40 = _grid(40)
    s2, x_T, w = 0.05 ** 2, np.array([0.9, -1.4, 0.3, 2.1]), FAMILY_CASES["three_mixed"]
    target = MU_U + sum(wi * (m - MU_U) for wi, m in zip(w, MUS))
    errs = []
    for a, p in ((a10, p10), (a40, p40)):
        end = _ddim_down(x_T.copy(), a, p, lambda x, ac: _compose([_eps_gauss(x, ac, m, s2) for m in MUS], _eps_gauss(x, ac, MU_U, s2), w))
        errs.append(float(np.abs(end - _ode_exact(x_T, a[-1], p[0], target, s2)).max()))
    assert errs[1] < errs[0]
