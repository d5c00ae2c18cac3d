"""CPU-side checks of DDIM editing (img2img start, keep-mask inpainting): the launcher in the header and in both builds, its argument
checks (no device is touched), its op kind in ABI 8, every refusal of `edit` with its name, the k-from-strength rule, the per-stage
min-pooled masks, the replay units of a chain that starts past row 0, and the order of the host-noise draws of a stage."""
import ctypes as C

import pytest
import torch

from golden_cfg import UNET_SMALL, VQ_SMALL, BERT_SMALL, frido_cfg
from frido_amd import _lib, patching, runtime, samplers


# ---- the launcher and the ABI ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_launcher_and_its_op_kind():
    assert "frido_keep_blend" in _lib.declared_symbols() and "frido_keep_blend" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 8
    assert _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36 and _lib.OP_KINDS["FRIDO_OP_ATTN_MH"] == 26
    assert C.sizeof(_lib.FridoOp) == 520 and C.sizeof(_lib.STRUCTS["FridoGemm"]) == 512
    assert C.sizeof(_lib.STRUCTS["FridoSamplerStep"]) == 232 and C.sizeof(_lib.STRUCTS["FridoDpmStep"]) == 112
    assert C.sizeof(_lib.STRUCTS["FridoQSample"]) == 112
    assert _lib.OP_KINDS["FRIDO_OP_KEEP_BLEND"] == 33 and _lib.KIND_STRUCT["FRIDO_OP_KEEP_BLEND"] == "FridoKeepBlend"
    assert C.sizeof(_lib.STRUCTS["FridoKeepBlend"]) == 120
    assert runtime.EDIT_RNG_STREAM == 64


@pytest.mark.parametrize("planes", ["f16", "bf16"])
def test_both_builds_export_the_launcher_and_agree_on_the_struct_size(planes):
    L = _lib.lib(planes)
    assert hasattr(L, "frido_keep_blend")
    assert L.frido_sizeof_desc(_lib.OP_KINDS["FRIDO_OP_KEEP_BLEND"]) == L.frido_sizeof_desc(33) == C.sizeof(_lib.STRUCTS["FridoKeepBlend"])
    assert L.frido_sizeof_desc(1001) == -1      # the kind-less descriptor code of ABI 7 is gone
    assert L.frido_abi_version() == 8


K_OK = dict(x=0x1000, z0=0x2000, mask=0x3000, qtab=0x4000, step=0x5000, B=3, HW=35, Cx=6, c0=3, c1=6, row_offset=2, rng_stream=65)


def test_an_accepted_descriptor_passes_the_argument_checks():
    """On a machine with the GPU the descriptor points at real buffers and the launch succeeds; without one the made-up addresses pass every
    check and the launch itself reports the missing device (FRIDO_EHIP), which is not an argument error."""
    L = _lib.lib()
    if torch.cuda.is_available():
        x, z0, m = torch.zeros(3, 35, 6, device="cuda"), torch.zeros(3, 35, 6, device="cuda"), torch.ones(3, 35, device="cuda")
        qtab, step = torch.ones(8, 2, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        d = _lib.STRUCTS["FridoKeepBlend"](**dict(K_OK, x=x.data_ptr(), z0=z0.data_ptr(), mask=m.data_ptr(), qtab=qtab.data_ptr(), step=step.data_ptr()))
        assert L.frido_keep_blend(C.byref(d), torch.cuda.current_stream().cuda_stream) == 0, L.frido_last_error()
        torch.cuda.synchronize()
        assert torch.isfinite(x).all()
    else:
        d = _lib.STRUCTS["FridoKeepBlend"](**K_OK)
        assert L.frido_keep_blend(C.byref(d), None) == -2 and b"frido_keep_blend:" not in L.frido_last_error()


@pytest.mark.parametrize("over, msg", [
    (dict(x=None), b"null pointer"), (dict(z0=None), b"null pointer"), (dict(qtab=None), b"coefficient table"),
    (dict(B=0), b"must be positive"), (dict(B=-1), b"must be positive"), (dict(HW=0), b"must be positive"), (dict(Cx=0), b"must be positive"),
    (dict(c0=-1), b"channel window"), (dict(c0=6), b"channel window"), (dict(c0=4, c1=4), b"channel window"), (dict(c1=7), b"channel window"),
    (dict(c0=2 ** 31 - 1), b"channel window"),
    (dict(row_offset=-1), b"row_offset"), (dict(clean=2), b"clean is 0 or 1"),
    (dict(noise=0x6000, noise_C=6), b"one noise form per launch"),                                   # rng_stream is set in K_OK
    (dict(noise=0x6000, noise_C=6, rng_stream=0, rng_dev=0x7000), b"one noise form per launch"),
    (dict(noise=0x6000, noise_C=6, rng_stream=0, seed=5), b"one noise form per launch"),
    (dict(noise=0x6000, noise_C=5, rng_stream=0), b"noise_C >= c1"),
    (dict(noise=0x6000, noise_C=6, rng_stream=0, noise_stride=-1), b"noise_stride >= 0"),
    (dict(clean=1, rng_stream=0, noise=0x6000, noise_C=6), b"clean = 1 reads no noise"),
    (dict(clean=1, rng_dev=0x7000), b"clean = 1 reads no noise"),
    (dict(HW=2 ** 31 - 1, Cx=12, c0=0, c1=12), b"32-bit group counter"),
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) if isinstance(o, dict) else None)
@pytest.mark.parametrize("planes", ["f16", "bf16"])
def test_keep_blend_rejects_bad_descriptors_without_touching_a_device(over, msg, planes):
    L = _lib.lib(planes)
    d = _lib.STRUCTS["FridoKeepBlend"](**dict(K_OK, **over))
    assert L.frido_keep_blend(C.byref(d), None) == -1, over
    err = L.frido_last_error()
    assert b"frido_keep_blend" in err and msg in err, err
    assert L.frido_keep_blend(None, None) == -1 and b"frido_keep_blend" in L.frido_last_error()


# ---- the public entry point's refusals ------------------------------------------------------------------------------------------------
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


def _edit(sampler, cond=CTX, z0=Z0, **kw):
    kw = dict(dict(t_start=3, num_stage=2, verbose=False), **kw)
    return sampler.edit(6, z0, cond, **kw)


def test_the_existing_refusals_of_sample_stay(model):
    for cls in (samplers.DDIMSampler, samplers.PLMSSampler, samplers.DPMSolverSampler):
        with pytest.raises(NotImplementedError, match="mask / x0"):
            cls(model).sample(S=6, batch_size=2, shape=(6, 16, 16), conditioning=CTX, num_stage=2, verbose=False, mask=torch.ones(2, 1, 16, 16), x0=Z0)


@pytest.mark.parametrize("name", ["PLMSSampler", "DPMSolverSampler"])
def test_the_other_samplers_refuse_edit_by_name(model, name):
    with pytest.raises(NotImplementedError, match=name):
        _edit(getattr(samplers, name)(model))


@pytest.mark.parametrize("kw, word", [
    (dict(score_corrector=object()), "score_corrector"), (dict(noise_dropout=0.1), "noise_dropout"),
    (dict(cond=dict(c_crossattn=[CTX])), "dict / list conditioning"), (dict(cond=[CTX]), "dict / list conditioning"),
    (dict(unconditional_conditioning=[CTX], unconditional_guidance_scale=2.0), "dict / list conditioning"),
])
def test_what_edit_cannot_honour_is_refused_by_name(model, kw, word):
    with pytest.raises(NotImplementedError, match=word):
        _edit(samplers.DDIMSampler(model), **kw)


def test_split_input_params_is_refused():
    m = _model()
    m.split_input_params = dict(ks=(8, 8), stride=(4, 4))
    with pytest.raises(NotImplementedError, match="split_input_params"):
        _edit(samplers.DDIMSampler(m))


@pytest.mark.parametrize("kw, word", [
    (dict(t_start=0), "t_start"), (dict(t_start=7), "t_start"), (dict(t_start=2.0), "t_start"), (dict(t_start=None), "exactly one"),
    (dict(strength=0.5), "exactly one"),
    (dict(keep_mask=torch.ones(2, 1, 8, 16)), "keep_mask must be"), (dict(keep_mask=torch.ones(2, 6, 16, 16)), "keep_mask must be"),
    (dict(keep_mask=torch.ones(2, 1, 16, 16, device="meta")), "keep_mask lives on"),
    (dict(first_stage=2), "first_stage"), (dict(first_stage=-1), "first_stage"), (dict(num_stage=1, first_stage=1), "first_stage"),
    (dict(init="noise"), "that is sample"), (dict(init="z0", x_T=Z0), "x_T is the start state"), (dict(init="x"), "init="), (dict(blend="all"), "blend="),
    (dict(init="noise", x_T=torch.zeros(2, 3, 16, 16)), "x_T must be"),
])
def test_bad_edit_arguments_are_value_errors(model, kw, word):
    with pytest.raises(ValueError, match=word):
        _edit(samplers.DDIMSampler(model), **kw)


def test_cpu_tensors_raise_the_hip_error(model):
    with pytest.raises(_lib.FridoHipError, match="no CPU path"):
        _edit(samplers.DDIMSampler(model))
    with pytest.raises(_lib.FridoHipError, match="no CPU path"):
        _edit(samplers.DDIMSampler(model), keep_mask=torch.ones(2, 1, 16, 16))


@pytest.mark.parametrize("S, strength, k", [(50, 0.5, 25), (50, 0.0, 1), (50, 0.001, 1), (50, 1.0, 50), (50, 1.7, 50), (6, 0.7, 4), (24, 0.99, 23), (3, 0.34, 1)])
def test_steps_from_strength(S, strength, k):
    """k = clamp(int(strength * S), 1, S)."""
    assert samplers.edit_steps(S, strength=strength) == k
    assert samplers.edit_steps(S, t_start=k) == k


# ---- stage masks ---------------------------------------------------------------------------------------------------------------------
def _hand_mask():
    m = torch.ones(1, 1, 8, 8)
    m[0, 0, 0, 0] = 0.0          # one regenerated pixel in the top-left 4 x 4 block
    m[0, 0, 5, 6] = 0.25         # a soft value in the block rows 4-5, columns 6-7
    m[0, 0, 2:4, 4:6] = 0.5      # a whole 2 x 2 block at one value
    return m


def test_stage_masks_two_stages():
    m = _hand_mask()
    coarse, fine = runtime.stage_masks(m, 2)
    assert fine is m
    want = torch.ones(4, 4)
    want[0, 0], want[2, 3], want[1, 2] = 0.0, 0.25, 0.5
    assert torch.equal(coarse[0, 0], want.repeat_interleave(2, 0).repeat_interleave(2, 1))
    assert bool((coarse <= m).all())          # a coarse cell is kept only where all of it is


def test_stage_masks_three_stages():
    m = _hand_mask()
    s0, s1, s2 = runtime.stage_masks(m, 3)
    assert s2 is m and torch.equal(s1, runtime.stage_masks(m, 2)[0])
    want = torch.tensor([[0.0, 0.5], [1.0, 0.25]])
    assert torch.equal(s0[0, 0], want.repeat_interleave(4, 0).repeat_interleave(4, 1))
    assert bool((s0 <= s1).all()) and bool((s1 <= s2).all())
    assert [tuple(t.shape) for t in (s0, s1, s2)] == [(1, 1, 8, 8)] * 3
    with pytest.raises(ValueError, match="does not split"):
        runtime.stage_masks(torch.ones(1, 1, 6, 8), 3)


# ---- replay units of a chain that starts past row 0 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, K, i0, log, want", [
    (23, 20, 0, 10 ** 9, [1, 20, 1, 1]),          # S = 24, k = 23: step 0 is logged, one 20-step unit, a remainder
    (23, 20, 1, 10 ** 9, [20, 1, 1]),             # the same after a first step run on its own
    (21, 20, 1, 10 ** 9, [20]),
    (20, 20, 1, 10 ** 9, [1] * 19),               # 19 steps left: no 20-step graph exists
    (45, 20, 1, 10 ** 9, [20, 20, 1, 1, 1, 1]),
    (6, 2, 1, 2, [1, 2, 2]),                      # index 4, 2, 0 are logged: steps 1, 3, 5 end their units
    (4, 20, 0, 100, [1, 1, 1, 1]),
])
def test_replay_units_with_a_start_offset(n, K, i0, log, want):
    units = runtime.replay_units(n, K, runtime.logged_at(n, log), i0)
    assert units == want and sum(units) == n - i0
    i = i0
    for u in units:          # a logged step only ever ENDS a unit
        assert not any(runtime.logged_at(n, log)(j) for j in range(i, i + u - 1))
        i += u


# ---- the order of the host-noise draws ---------------------------------------------------------------------------------------------------
class _StubEngine(runtime.SamplerEngine):
    """SamplerEngine._edit_stage with everything that touches the device replaced by a recorder."""

    def __init__(self, S):
        self.B, self.C, self.H, self.W, self.embed, self.num_stage, self.n_steps = 2, 6, 4, 4, [3, 3], 2, S
        self.graphs, self.use_graph, self.uploads, self.events = {}, True, {}, []
        from types import SimpleNamespace
        self.stages = [SimpleNamespace(pre=SimpleNamespace(ops=["pre"]))] * 2

    def _upload_noise(self, s, tape, row0=0, key=None):
        self.uploads[s if key is None else key] = (row0, [int(t.flatten()[0]) for t in tape])
        return 0, sum(self.embed[:s + 1])

    def _blend_op(self, s, window, masked, noise=None, clean=False):
        return ("blend", window, masked, clean)

    def _eval_ops(self, s):
        return ["eval"]

    def _update_op(self, s, noise=None, **kw):
        return ("update", s)

    def _prog(self, ops):
        eng = self

        class P:
            def run(self, sp):
                eng.events.append(("run", ops))
        return P()

    def _body(self, key, sp, build_ops):
        self.graphs.setdefault(key, build_ops())
        return self.graphs[key]

    def _go(self, g, sp):
        self.events.append(("go", g))

    def _log(self, s, i, sp, o):
        self.events.append(("log", i))

    def _replay(self, key, K, host_at, sp, after_unit=None, n=None, i0=0, **kw):
        self.events.append(("replay", key, n, i0))


def _draws():
    count = [0]

    def draw(shape):
        count[0] += 1
        draw.shapes.append(tuple(shape))
        return torch.full(shape, float(count[0]))
    draw.shapes = []
    return draw


def _stage(S, k, s, **spec):
    from types import SimpleNamespace
    eng, draw = _StubEngine(S), _draws()
    ed = runtime.EditSpec(None, k, None, None, **spec)
    o = SimpleNamespace(edit=ed, n=k, row0=S - k, draw=draw, log_every_t=10 ** 9, callback=None, img_callback=None, seed=0, sample0=0)
    eng._edit_stage(s, None, o)
    return eng, draw


def test_host_noise_order_masked_img2img():
    """init "z0" with a mask: the start draw, then step 0's update draw (its blend is the start draw itself), then blend and update
    alternating -- every draw (B, e_s, H, W), uploaded at the chain's start row."""
    eng, draw = _stage(6, 4, 1, masks=[None, None], init="z0")
    assert draw.shapes == [(2, 6, 4, 4)] * 8
    assert eng.uploads[("blend", 1)] == (2, [1, 3, 5, 7]) and eng.uploads[1] == (2, [2, 4, 6, 8])
    kinds = [e[0] for e in eng.events]
    assert kinds == ["run", "go", "log", "replay", "run"]
    assert eng.events[0][1] == [("blend", (3, 6), False, False)]                      # the start: an unmasked q_sample of the window
    assert eng.events[1][1] == [["eval"], ("update", 1), 1]                           # step 0: the plain body
    assert eng.events[3] == ("replay", ("edit_tape", 1), 4, 1)
    assert eng.graphs[("edit_tape", 1)] == [("blend", (3, 6), True, False), ["eval"], ("update", 1), 1]
    assert eng.events[4][1] == [("blend", (3, 6), True, True)]                        # reimpose: the clean blend under the mask


def test_host_noise_order_inpainting_from_noise_in_the_reference_form():
    """init "noise": no start draw; per step the blend's draw (q_sample's randn_like) before the update's (ddim.py:158-161 before
    p_sample_ddim).  blend "reference": the window is [0, e_s) and the body has a key of its own."""
    eng, draw = _stage(4, 4, 1, masks=[None, None], init="noise", blend="reference", reimpose=False)
    assert draw.shapes == [(2, 6, 4, 4)] * 8
    assert eng.uploads[("blend", 1)] == (0, [1, 3, 5, 7]) and eng.uploads[1] == (0, [2, 4, 6, 8])
    assert [e[0] for e in eng.events] == ["replay"] and eng.events[0] == ("replay", ("edit_tape_ref", 1), 4, 0)
    # the blend rewrites the frozen channels the stage's hoisted invariants come from: `pre` runs again in front of every evaluation
    assert eng.graphs[("edit_tape_ref", 1)] == [("blend", (0, 6), True, False), ["pre"], ["eval"], ("update", 1), 1]


def test_host_noise_order_plain_img2img_stage_0():
    """No mask: one start draw, then the updates' draws; the plain DDIM body serves every step; stage 0 draws its 3 channels."""
    eng, draw = _stage(6, 2, 0, masks=None, init="z0")
    assert draw.shapes == [(2, 3, 4, 4)] * 3
    assert eng.uploads[("blend", 0)] == (4, [1, 0]) and eng.uploads[0] == (4, [2, 3])
    assert [e[0] for e in eng.events] == ["run", "replay"] and eng.events[1] == ("replay", ("ddim_tape", 0), 2, 0)
    assert eng.events[0][1] == [("blend", (0, 3), False, False)] and list(eng.graphs) == [("ddim_tape", 0)]
