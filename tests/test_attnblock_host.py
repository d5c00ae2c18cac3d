"""CPU-side checks of the AttentionBlock denoiser family (use_spatial_transformer=False; pyunet.py:303-358): the parameter tree and the
per-site head counts against what the reference's own modules report (fixtures of tests/golden/make_golden_attnblock.py), the options
that are refused at construction, and the messages the denoiser keeps for what it was not built for."""
import pytest
import torch

from helpers import golden
from golden_cfg import UNET_SMALL
from attnblock_cfg import FORWARD, AB_SMALL, AB_FULL, AB_CLS_EMB
from frido_amd.arch import unet_arch
from frido_amd.models import PyUNetModel


@pytest.mark.parametrize("name", sorted(FORWARD))
def test_state_dict_and_head_counts_match_the_reference(name):
    g, cfg = golden(name), FORWARD[name]
    m = PyUNetModel(**cfg)
    sd = m.state_dict()
    assert sorted(sd) == [str(k) for k in g["keys"]]
    assert sum(v.numel() for v in sd.values()) == int(g["nparam"])
    sites = m.arch.attention_sites()
    assert [b.kind for b in sites] == ["attn"] * len(g["heads"])
    assert [b.heads for b in sites] == g["heads"].tolist()
    assert [b.new_order for b in sites] == g["new_order"].tolist()
    assert m.arch.context_dim is None
    # shapes of the new parameter kinds: Conv1d weights [out, in, 1]
    pre = sites[0].prefix
    C = sites[0].cin
    assert tuple(sd[pre + ".qkv.weight"].shape) == (3 * C, C, 1) and tuple(sd[pre + ".proj_out.weight"].shape) == (C, C, 1)
    if cfg.get("num_classes"):
        want = (cfg["num_classes"], 4 * cfg["model_channels"]) if cfg["use_embed"] else (4 * cfg["model_channels"], cfg["num_classes"])
        assert tuple(sd["label_emb.weight"].shape) == want and ("label_emb.bias" in sd) == (not cfg["use_embed"])


def test_head_counts_follow_the_reference_rules():
    heads = lambda cfg: [b.heads for b in unet_arch(cfg).attention_sites()]
    assert heads(AB_SMALL) == [2, 3, 3, 3, 3, 2, 2]                    # 64 / 96 channels at 32 per head
    assert heads(AB_FULL)[:3] == [12, 12, 18] and max(heads(AB_FULL)) == 30 and set(heads(AB_FULL)) == {12, 18, 30}
    # legacy=True forces ONE head on the input path and in the middle, the output path takes num_heads_upsample (pyunet.py:764)
    one = dict(AB_SMALL, num_head_channels=-1, num_heads=4, num_heads_upsample=1)
    assert set(heads(one)) == {1}
    up2 = dict(AB_SMALL, model_channels=64, num_head_channels=-1, num_heads=4, num_heads_upsample=2)      # 128 / 192 channels, output path: 2 heads of 64 / 96
    with pytest.raises(NotImplementedError, match="32, 64"):
        unet_arch(up2)
    # legacy=False: num_heads heads of C / num_heads channels everywhere
    assert set(heads(dict(AB_SMALL, channel_mult=[1, 2, 2], num_head_channels=-1, num_heads=2, legacy=False))) == {2}       # 64 channels: 2 x 32


def test_unsupported_head_dimensions_are_refused_at_construction():
    # num_heads=4, legacy=False at 192 channels: d = 48
    with pytest.raises(NotImplementedError, match=r"4 heads of 48 channels.*32, 64"):
        PyUNetModel(**dict(AB_SMALL, model_channels=64, num_head_channels=-1, num_heads=4, legacy=False))
    # the same option with legacy=True and the default num_heads_upsample: one head going down, 4 heads of 16 / 24 channels coming up
    with pytest.raises(NotImplementedError, match="32, 64"):
        PyUNetModel(**dict(AB_SMALL, num_head_channels=-1, num_heads=4))


def test_options_that_stay_out_of_scope_name_themselves():
    for opt in ("use_scale_shift_norm", "resblock_updown", "use_pos_embed", "use_mscond", "use_stage_expert"):
        with pytest.raises(NotImplementedError, match=opt):
            PyUNetModel(**dict(AB_SMALL, **{opt: True}))
    with pytest.raises(NotImplementedError, match="n_embed"):
        PyUNetModel(**dict(AB_SMALL, n_embed=16))
    with pytest.raises(NotImplementedError, match="dims"):
        PyUNetModel(**dict(AB_SMALL, dims=3))
    with pytest.raises(NotImplementedError, match="multi-head SpatialTransformer"):
        PyUNetModel(**dict(UNET_SMALL, legacy=False))
    with pytest.raises(AssertionError):
        PyUNetModel(**dict(AB_SMALL, context_dim=64))              # pyunet.py:516-517


def test_pinned_messages_stay():
    x, t = torch.zeros(2, 3, 16, 16), torch.tensor([1, 2])
    u = PyUNetModel(**UNET_SMALL)
    with pytest.raises(NotImplementedError, match="class-conditional"):
        u(x, t, context=torch.zeros(2, 5, 64), y=torch.tensor([1, 2]), stage=0)
    with pytest.raises(NotImplementedError, match="without a context"):
        u(x, t, stage=0)
    a = PyUNetModel(**AB_SMALL)
    with pytest.raises(NotImplementedError, match="class-conditional"):       # built without num_classes: takes no y
        a(x, t, y=torch.tensor([1, 2]), stage=0)
    c = PyUNetModel(**AB_CLS_EMB)
    with pytest.raises(ValueError, match="if and only if"):
        c(x, t, stage=0)
