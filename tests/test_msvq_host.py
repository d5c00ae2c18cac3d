"""CPU-side checks of MSFPNVQModel (the MS-VQGAN as a model of its own, taming/models/msvqgan.py:16-318): the three shipped msvqgan
configs instantiate, the state_dict key set is the reference's (msvq_small.npz), every refusal says its name, CPU tensors raise, the
codebook-loss launcher is declared / exported by both builds and rejects bad descriptors without touching a device, its op kind in ABI 8."""
import ctypes as C
import json
import os

import pytest
import torch

from helpers import golden, GOLDEN
from golden_cfg import VQ_SMALL
from frido_amd import _lib
from frido_amd._lib import FridoHipError

SHIPPED = json.load(open(os.path.join(GOLDEN, "shipped_msvq_cfgs.json")))
DUMMY = dict(target="taming.modules.losses.DummyLoss")


def _model(**over):
    from frido_amd.models import MSFPNVQModel
    return MSFPNVQModel(**dict(dict(VQ_SMALL, lossconfig=DUMMY), **over)).eval()


@pytest.fixture(scope="module")
def model():
    return _model()


def test_three_msvqgan_configs_are_recorded():
    assert sorted(SHIPPED) == ["msvqgan/msvqgan_f16f8_coco.yaml", "msvqgan/msvqgan_f16f8_openimage.yaml", "msvqgan/msvqgan_f8f4_openimage.yaml"]


@pytest.mark.parametrize("name", sorted(SHIPPED))
def test_shipped_msvqgan_config_instantiates(name):
    """The `model:` tree as shipped: target taming.models.msvqgan.MSFPNVQModel, lossconfig VQLPIPSWithDiscriminator (replaced by the no-op
    loss holder: its LPIPS weights are a download)."""
    from frido_amd.models import instantiate_from_config, MSFPNVQModel, DummyLoss
    cfg = SHIPPED[name]
    assert cfg["target"] == "taming.models.msvqgan.MSFPNVQModel"
    m = instantiate_from_config(cfg)
    assert isinstance(m, MSFPNVQModel) and isinstance(m.loss, DummyLoss)
    p = cfg["params"]
    assert m.embed_dim == list(p["embed_dim"]) and m.n_embed == list(p["n_embed"]) and m.monitor == p["monitor"]
    assert m.post_quant_conv.weight.shape[:2] == (p["ddconfig"]["z_channels"], sum(p["embed_dim"]))
    assert [q.embedding.weight.shape for q in m.ms_quantize] == [(n, e) for n, e in zip(p["n_embed"], p["embed_dim"])]
    assert len(m.res_list) == p["edconfig"]["multiscale"] and m.get_last_layer() is m.decoder.conv_out.weight


def test_import_path_of_the_reference():
    from taming.models.msvqgan import MSFPNVQModel, VQModelInterface
    import frido_amd.models as M
    assert MSFPNVQModel is M.MSFPNVQModel and VQModelInterface is M.VQModelInterface
    assert not issubclass(M.VQModelInterface, M.MSFPNVQModel)      # a class next to it: VQModelInterface is not re-parented


def test_state_dict_keys_are_the_references(model):
    keys = sorted(model.state_dict())
    assert keys == list(golden("msvq_small")["keys"])
    from frido_amd.models import VQModelInterface
    assert keys == sorted(VQModelInterface(**VQ_SMALL, lossconfig=DUMMY).state_dict())      # the same weights load into either


def test_constructor_keeps_the_options():
    m = _model(use_aux_loss=True, sane_index_shape=True, quant_beta=0.4, legacy=False, image_key="img", monitor="val/rec_loss",
               lossconfig=dict(target="taming.modules.losses.vqperceptual.VQLPIPSWithDiscriminator", params=dict(disc_start=1)))
    assert (m.use_aux_loss, m.sane_index_shape, m.quant_beta, m.legacy, m.image_key, m.monitor) == (True, True, 0.4, False, "img", "val/rec_loss")
    assert m.vq_cfg["quant_beta"] == 0.4 and m.vq_cfg["legacy"] is False and m.fusion == "concat" and m.unsample_type == "nearest"
    assert m.test_step({}, 0) is None


X = torch.zeros(2, 3, 64, 64)


def test_cpu_tensors_raise_the_hip_error(model):
    for call in (lambda: model.encode(X), lambda: model(X), lambda: model.decode(torch.zeros(2, 6, 16, 16)),
                 lambda: model.log_images(dict(image=torch.zeros(2, 64, 64, 3)))):
        with pytest.raises(FridoHipError, match="no CPU fallback"):
            call()


def test_get_input_and_img_ids(model):
    img = torch.arange(2 * 4 * 5 * 3, dtype=torch.float64).reshape(2, 4, 5, 3)
    x = model.get_input(dict(image=img), "image")
    assert x.dtype == torch.float32 and x.shape == (2, 3, 4, 5) and x.is_contiguous() and torch.equal(x, img.permute(0, 3, 1, 2).float())
    assert model.get_input(dict(image=img[..., 0]), "image").shape == (2, 1, 4, 5)
    assert model.get_img_ids(dict(file_name=["a", "b"])) == ["a", "b"]


# ---- refusals: by name, never ignored -------------------------------------------------------------------------------------------------
def test_training_entry_points_say_there_is_no_backward_pass(model):
    with pytest.raises(FridoHipError, match="training_step: no backward pass"):
        model.training_step({}, 0, 0)
    with pytest.raises(FridoHipError, match="configure_optimizers: no backward pass"):
        model.configure_optimizers()


def test_validation_step_names_the_part_that_exists(model):
    with pytest.raises(NotImplementedError, match=r"validation_step.*LPIPS.*encode\(\)\[1\]"):
        model.validation_step({}, 0)


def test_decode_code_is_refused_like_the_reference(model):
    with pytest.raises(NotImplementedError, match=r"decode_code.*self\.quantize.*AttributeError.*force_codes"):
        model.decode_code(torch.zeros(2, 64, dtype=torch.long))


@pytest.mark.parametrize("over,name", [
    (dict(remap="x.npy"), "remap"), (dict(fusion="sum"), "fusion='sum'"), (dict(colorize_nlabels=5), "colorize_nlabels"),
    (dict(edconfig=dict(VQ_SMALL["edconfig"], double_z=True)), "double_z=True"),
], ids=["remap", "fusion", "colorize_nlabels", "double_z"])
def test_constructor_options_that_are_not_built_are_refused(over, name):
    with pytest.raises(NotImplementedError, match=name):
        _model(**over)


def test_more_than_three_input_channels_are_refused(model):
    x = torch.zeros(1, 5, 64, 64)
    for call in (lambda: model.encode(x), lambda: model(x), lambda: model.log_images(dict(image=x.permute(0, 2, 3, 1)))):
        with pytest.raises(NotImplementedError, match="more than 3 channels.*to_rgb"):
            call()


# ---- the launcher -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_launcher_and_its_op_kind():
    assert "frido_vq_commit_loss" in _lib.declared_symbols() and "frido_vq_commit_loss" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 8
    assert _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36 and _lib.OP_KINDS["FRIDO_OP_ATTN_MH"] == 26
    assert C.sizeof(_lib.FridoOp) == 520 and C.sizeof(_lib.STRUCTS["FridoGemm"]) == 512 and C.sizeof(_lib.STRUCTS["FridoVq"]) == 80
    assert _lib.OP_KINDS["FRIDO_OP_VQ_COMMIT_LOSS"] == 31 and _lib.KIND_STRUCT["FRIDO_OP_VQ_COMMIT_LOSS"] == "FridoVqCommitLoss"
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        assert L.frido_abi_version() == 8
        assert L.frido_sizeof_desc(31) == C.sizeof(_lib.STRUCTS["FridoVqCommitLoss"]) and hasattr(L, "frido_vq_commit_loss")
    assert C.sizeof(_lib.STRUCTS["FridoVqCommitLoss"]) == 184
    assert _lib.VQLOSS_MAX_SCALES == 4 and _lib.VQLOSS_WS_BYTES == 4 * 256 * 8


def test_both_builds_export_the_launcher():
    for planes in ("f16", "bf16"):
        assert hasattr(_lib.lib(planes), "frido_vq_commit_loss"), planes


def test_launcher_is_an_op_kind_for_captured_programs():
    d = _desc()
    assert _lib.op_of("FRIDO_OP_VQ_COMMIT_LOSS", d) == (31, d)


def _desc(n=2, **over):
    from frido_amd.vqloss import commit_loss_desc
    scales = [(0x1000 * (k + 1), 0x10000 * (k + 1), 128 << (2 * k), 6, 3, 3) for k in range(n)]
    d = commit_loss_desc(scales, partials=0x100000, out=0x200000, emb_loss=0x300000, beta=0.25, legacy=True)
    d.n_scales = n                      # (commit_loss_desc fills at most 4 scales; the count is what the launcher must check)
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


@pytest.mark.parametrize("n,over", [
    (2, dict(e=(1, 0))), (2, dict(e=(0, -3))), (5, {}), (0, {}), (2, dict(z=(1, None))), (2, dict(zq=(0, None))), (2, dict(partials=None)),
    (2, dict(out=None)), (2, dict(emb_loss=None)), (2, dict(npix=(1, 0))), (2, dict(C=(0, 0))), (2, dict(c0=(0, -1))), (2, dict(c0=(1, 4))),
    (2, dict(beta=float("nan"))),
    (1, dict(C=(0, 8), c0=(0, 4), e=(0, 4), z=(0, 0x1004))),      # the 16-byte path needs aligned maps
], ids=lambda o: str(o))
def test_launcher_rejects_bad_descriptors_without_touching_a_device(n, over):
    L = _lib.lib()
    assert L.frido_vq_commit_loss(C.byref(_desc(n, **over)), None) == -1, (n, over)
    assert b"frido_vq_commit_loss" in L.frido_last_error()


def test_null_descriptor_is_rejected():
    L = _lib.lib()
    assert L.frido_vq_commit_loss(None, None) == -1 and b"frido_vq_commit_loss" in L.frido_last_error()
