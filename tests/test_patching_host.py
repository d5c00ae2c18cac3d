"""CPU-side checks of the patch-wise mode (FridoDiffusion.split_input_params): the weighting / normalization tables against the reference's
own tensors (patch_apply.npz, patch_vq.npz), the crop grid and the clamping rules, every refusal with its message, the new launchers in the
header, the launchers' argument checks (no device is touched) and their op kinds in ABI 8."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import golden
from golden_cfg import VQ_SMALL, BERT_SMALL, frido_cfg
from patch_cfg import MODELS, SPLIT, SPLIT_TIE, SPLIT_RECT, RECT_HW, SPLIT_ENC, COND_STAGE_KEY
from frido_amd import _lib, patching


@pytest.mark.parametrize("tag,split,hw,mode,file", [
    ("notie", SPLIT, (16, 16), patching.MODEL, "patch_apply"), ("tie", SPLIT_TIE, (16, 16), patching.MODEL, "patch_apply"),
    ("rect", SPLIT_RECT, RECT_HW, patching.MODEL, "patch_apply"), ("dec", SPLIT, (16, 16), patching.DECODE, "patch_vq"),
    ("enc", SPLIT_ENC, (64, 64), patching.ENCODE, "patch_vq")])
def test_tables_are_bit_identical_to_the_reference(tag, split, hw, mode, file):
    g = golden(file)
    geo = patching.geometry(split, hw[0], hw[1], mode, None)
    assert geo.weighting.dtype == torch.float32 and geo.normalization.dtype == torch.float32
    assert np.array_equal(geo.weighting.numpy(), g[f"{tag}_weighting"]), tag
    assert np.array_equal(geo.normalization.numpy(), g[f"{tag}_normalization"]), tag
    assert geo.weighting.shape == (geo.out[2] * geo.out[3], geo.L) and geo.normalization.shape == geo.out[:2]


def test_crop_grid_origins_and_cover():
    geo = patching.geometry(SPLIT, 16, 16, patching.MODEL, None)
    assert (geo.Ly, geo.Lx, geo.L, geo.max_cover) == (3, 3, 9, 4)
    assert geo.origins() == [(y, x) for y in (0, 4, 8) for x in (0, 4, 8)]
    # nn.Unfold's crop order: crop l of the unfolded index map starts at origins()[l]
    idx = torch.arange(16 * 16, dtype=torch.float32).view(1, 1, 16, 16)
    u = torch.nn.Unfold(kernel_size=(8, 8), stride=(4, 4))(idx).view(8, 8, 9)
    assert [(int(v) // 16, int(v) % 16) for v in u[0, 0]] == geo.origins()
    rect = patching.geometry(SPLIT_RECT, *RECT_HW, patching.MODEL, None)
    assert (rect.Ly, rect.Lx, rect.L, rect.max_cover) == (3, 4, 12, 2) and rect.origins()[5] == (4, 4)
    one = patching.geometry(dict(SPLIT, ks=(16, 16), stride=(16, 16)), 16, 16, patching.MODEL, None)
    assert one.L == 1 and one.max_cover == 1
    # the same geometry comes from the cache; another clip value is another geometry
    assert patching.geometry(dict(SPLIT), 16, 16, patching.MODEL, None) is geo
    assert patching.geometry(dict(SPLIT, clip_max_weight=0.4), 16, 16, patching.MODEL, None) is not geo


def test_decode_and_encode_geometry_scale_and_clamp():
    dec = patching.geometry(SPLIT, 16, 16, patching.DECODE, None)
    assert dec.src == (16, 16, 8, 8, 4, 4) and dec.out == (64, 64, 32, 32, 16, 16) and dec.L == 9
    enc = patching.geometry(SPLIT_ENC, 64, 64, patching.ENCODE, None)
    assert enc.src == (64, 64, 32, 32, 16, 16) and enc.out == (16, 16, 8, 8, 4, 4)
    # frido.py:846-852: a ks / stride larger than the tensor is clamped to it (one crop)
    big = patching.geometry(dict(SPLIT, ks=(128, 128), stride=(64, 64)), 16, 16, patching.DECODE, None)
    assert big.src == (16, 16, 16, 16, 16, 16) and big.L == 1
    with pytest.raises(ValueError, match="square ks"):
        patching.geometry(dict(SPLIT, ks=(4, 8)), 16, 16, patching.DECODE, None)
    with pytest.raises(ValueError, match="square ks"):
        patching.geometry(dict(SPLIT_ENC, ks=(16, 32)), 64, 64, patching.ENCODE, None)
    with pytest.raises(ValueError, match="multiples of vqf"):
        patching.geometry(dict(SPLIT_ENC, ks=(30, 30), stride=(17, 17)), 64, 64, patching.ENCODE, None)


def test_geometries_the_reference_cannot_stitch_raise():
    with pytest.raises(ValueError, match="do not tile .* NaN"):
        patching.geometry(dict(SPLIT, stride=(3, 3)), 16, 16, patching.MODEL, None)
    with pytest.raises(ValueError, match="do not tile"):
        patching.geometry(dict(SPLIT, ks=(8, 8), stride=(4, 4)), 16, 18, patching.MODEL, None)
    with pytest.raises(ValueError, match="larger than the 16 x 16 latent"):
        patching.geometry(dict(SPLIT, ks=(32, 32)), 16, 16, patching.MODEL, None)
    with pytest.raises(ValueError, match="not finite and positive"):      # tie_braker on a single row of crops: delta_border(1, Lx) is 0 / 0
        patching.geometry(dict(SPLIT_TIE, ks=(16, 8)), 16, 16, patching.MODEL, None)
    with pytest.raises(KeyError, match="tie_braker"):
        patching.geometry({k: v for k, v in SPLIT.items() if k != "tie_braker"}, 16, 16, patching.MODEL, None)


def _model(ucfg=MODELS["plain"], key="crossattn", **over):
    from frido_amd.models import instantiate_from_config
    cfg = dict(frido_cfg(ucfg, VQ_SMALL, BERT_SMALL), cond_stage_key=COND_STAGE_KEY, **over)
    cfg["cond_stage_config"], cfg["cond_stage_trainable"], cfg["conditioning_key"] = "__is_unconditional__", False, key
    m = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
    m.model.conditioning_key = key
    m.split_input_params = dict(SPLIT)
    return m


def test_refusals_name_split_input_params():
    from frido.models.diffusion.ddim import DDIMSampler
    from frido.models.diffusion.plms import PLMSSampler
    m = _model()
    x, t, c = torch.zeros(2, 6, 16, 16), torch.tensor([5, 5]), torch.zeros(2, 5, 64)
    # ancestral sampling
    for call in (lambda: m.p_sample(x, c, t, 1), lambda: m.p_mean_variance(x, c, t, 1, clip_denoised=False),
                 lambda: m.p_sample_loop(c, (2, 6, 16, 16)), lambda: m.progressive_denoising(c, (2, 6, 16, 16)),
                 lambda: m.sample(c, batch_size=2)):
        with pytest.raises(NotImplementedError, match="ancestral sampling .*split_input_params"):
            call()

    class Corrector:
        def modify_score(self, *a, **k):
            raise AssertionError("never reached")
    for cls in (DDIMSampler, PLMSSampler):
        with pytest.raises(NotImplementedError, match="score_corrector .*split_input_params"):
            cls(m).sample(S=2, batch_size=2, shape=(6, 16, 16), conditioning=c, num_stage=2, verbose=False, score_corrector=Corrector())
        with pytest.raises(NotImplementedError, match="dict / list conditioning .*split_input_params"):
            cls(m).sample(S=2, batch_size=2, shape=(6, 16, 16), conditioning={"c_crossattn": [c]}, num_stage=2, verbose=False)
        with pytest.raises(ValueError, match="do not tile"):
            cls(m).sample(S=2, batch_size=2, shape=(6, 18, 16), conditioning=c, num_stage=2, verbose=False)
        with pytest.raises(NotImplementedError, match="dict / list conditioning .*split_input_params"):
            cls(m).sample(S=2, batch_size=2, shape=(6, 16, 16), conditioning=c, num_stage=2, verbose=False, unconditional_guidance_scale=1.5,
                          unconditional_conditioning=[c])
    # conditionings
    for key in ("concat", "hybrid"):      # not on the reference's list: a full-size c_concat does not fit the crops
        mk = _model(key=key)
        with pytest.raises(NotImplementedError, match=f"conditioning_key='{key}' .*split_input_params"):
            mk.apply_model(x, t, c, stage=1)
        with pytest.raises(NotImplementedError, match=f"conditioning_key='{key}' .*split_input_params"):
            DDIMSampler(mk).sample(S=2, batch_size=2, shape=(6, 16, 16), conditioning=c, num_stage=2, verbose=False)
    for cond in ({"c_crossattn": [c]}, [c]):
        with pytest.raises(NotImplementedError, match="dict / list conditioning .*split_input_params"):
            m.apply_model(x, t, cond, stage=1)
    for key in patching.UNFOLDED_COND_KEYS:
        m.cond_stage_key = key
        with pytest.raises(NotImplementedError, match=f"cond_stage_key='{key}' .*unfolds the conditioning.*split_input_params"):
            m.apply_model(x, t, c, stage=1)
    m.cond_stage_key = "coordinates_bbox"
    with pytest.raises(NotImplementedError, match="coordinates_bbox.*split_input_params"):
        m.apply_model(x, t, c, stage=1)
    m.cond_stage_key = COND_STAGE_KEY
    with pytest.raises(ValueError, match="return_ids.*split_input_params"):
        m.apply_model(x, t, c, stage=1, return_ids=True)
    # geometry
    with pytest.raises(ValueError, match="larger than the 4 x 4 latent"):
        m.apply_model(torch.zeros(2, 6, 4, 4), t, c, stage=1)
    with pytest.raises(ValueError, match="do not tile"):
        m.apply_model(torch.zeros(2, 6, 16, 18), t, c, stage=1)
    m.split_input_params = dict(SPLIT, ks=(4, 8))
    with pytest.raises(ValueError, match="square ks"):
        m.decode_first_stage(torch.zeros(2, 6, 16, 16))
    with pytest.raises(ValueError, match="square ks"):
        m.encode_first_stage(torch.zeros(2, 3, 64, 64))
    m.split_input_params = dict(SPLIT)
    with pytest.raises(NotImplementedError, match="return_code .*split_input_params"):
        m.decode_first_stage(torch.zeros(2, 6, 16, 16), return_code=True)
    # past every refusal the path needs the GPU: there is no CPU fallback, and nothing fell through to the whole-latent call silently
    with pytest.raises(_lib.FridoHipError, match="no CPU"):
        m.apply_model(x, t, c, stage=1)
    with pytest.raises(_lib.FridoHipError, match="no CPU"):
        m.encode_first_stage(torch.zeros(2, 3, 64, 64))
    assert tuple(m.split_input_params["original_image_size"]) == (64, 64)      # frido.py:968


def test_patch_distributed_vq_false_leaves_the_first_stage_whole():
    """frido.py:878-882, 995-996: without patch_distributed_vq decode / encode take the whole tensor (here: up to the device check, with a
    geometry that would be refused if it were looked at)."""
    m = _model()
    m.split_input_params = dict(SPLIT, ks=(4, 8), patch_distributed_vq=False)
    with pytest.raises(_lib.FridoHipError, match="VQModelInterface.decode"):
        m.decode_first_stage(torch.zeros(2, 6, 16, 16))
    with pytest.raises(_lib.FridoHipError, match="VQModelInterface.encode"):
        m.encode_first_stage(torch.zeros(2, 3, 64, 64))
    assert "original_image_size" not in m.split_input_params


def test_header_declares_the_new_launchers_and_their_op_kinds():
    declared = _lib.declared_symbols()
    for name in ("frido_unfold", "frido_fold", "frido_capture_begin", "frido_capture_end"):
        assert name in declared and name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 8
    assert _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36 and _lib.OP_KINDS["FRIDO_OP_ATTN_MH"] == 26
    assert C.sizeof(_lib.FridoOp) == 520
    assert C.sizeof(_lib.STRUCTS["FridoSamplerStep"]) == 232
    assert _lib.OP_KINDS["FRIDO_OP_UNFOLD"] == 27 and _lib.KIND_STRUCT["FRIDO_OP_UNFOLD"] == "FridoUnfold"
    assert _lib.OP_KINDS["FRIDO_OP_FOLD"] == 28 and _lib.KIND_STRUCT["FRIDO_OP_FOLD"] == "FridoFold"
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        assert L.frido_abi_version() == 8
        assert L.frido_sizeof_desc(27) == C.sizeof(_lib.STRUCTS["FridoUnfold"]) and hasattr(L, "frido_unfold")
        assert L.frido_sizeof_desc(28) == C.sizeof(_lib.STRUCTS["FridoFold"]) and hasattr(L, "frido_fold")
    assert C.sizeof(_lib.STRUCTS["FridoUnfold"]) == 48 and C.sizeof(_lib.STRUCTS["FridoFold"]) == 80


def test_launchers_check_their_arguments_before_touching_a_device():
    L = _lib.lib()
    for planes in ("f16", "bf16"):
        assert hasattr(_lib.lib(planes), "frido_fold") and hasattr(_lib.lib(planes), "frido_capture_end")
    geo = patching.geometry(SPLIT, 16, 16, patching.MODEL, None)
    ok = geo.unfold_desc(0x1000, 0x2000, 2, 3)
    assert (ok.H, ok.W, ok.kh, ok.kw, ok.sy, ok.sx, ok.B, ok.C) == (16, 16, 8, 8, 4, 4, 2, 3)
    bad = [dict(src=None), dict(dst=None), dict(B=0), dict(C=0), dict(sy=3), dict(kw=32), dict(sx=0)]
    for over in bad:
        d = geo.unfold_desc(0x1000, 0x2000, 2, 3)
        for k, v in over.items():
            setattr(d, k, v)
        assert L.frido_unfold(C.byref(d), None) != 0, over
        assert b"frido_unfold" in L.frido_last_error()
    F = _lib.STRUCTS["FridoFold"]
    base = dict(crops=0x1000, out=0x2000, wt=0x3000, norm=0x4000, B=2, H=16, W=16, C=3, kh=8, kw=8, sy=4, sx=4)
    for over in (dict(crops=None), dict(wt=None), dict(norm=None), dict(out=None), dict(sy=5), dict(kh=17), dict(out_u8=0x5000, u8_mode=0),
                 dict(out_u8=0x5000, u8_mode=3)):
        assert L.frido_fold(C.byref(F(**dict(base, **over))), None) != 0, over
        assert b"frido_fold" in L.frido_last_error()
    assert L.frido_capture_end(None, None) != 0
