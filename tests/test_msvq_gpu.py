"""MSFPNVQModel on the MI355X against the reference's own results (tests/golden/msvq_small.npz, msvq_small_nl.npz: VQ_SMALL at B = 2 on
64 x 64 images, latents 8 x 8 and 16 x 16, made by tests/golden/make_golden_msvq.py from taming/models/msvqgan.py).

Bounds are the ones the existing first-stage tests of tests/test_model_gpu.py apply to the same model:
  ENC  5e-4 of max |.|   test_vq_encode_matches_reference_golden's bound on the pre-quant latent h -- here on quant, whose codes must be EQUAL
                         (every decision of the fixture is clear by more than 1e-3 relative: its `margin_*`), so no pixel is excused;
  PIX  2e-4 of max |.|   test_vq_decode_matches_reference_golden's bound on the decoded image (2e-3 on the bf16-pair build:
                         test_vq_decode_heavy_profile_both_plane_formats);
  emb_loss               2 * ENC-as-absolute / rms(z_q - z): a mean of squares doubles a relative perturbation of its argument.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import golden  # noqa: E402
from golden_cfg import VQ_SMALL  # noqa: E402
from frido_amd.synth import fill_module  # noqa: E402

ENC, PIX, PIX_BF16P = 5e-4, 2e-4, 2e-3
DUMMY = dict(target="taming.modules.losses.DummyLoss")
E = VQ_SMALL["embed_dim"]


def _rel(got, ref):
    ref = torch.as_tensor(ref).double()
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def _make(**over):
    from frido_amd.models import MSFPNVQModel
    return fill_module(MSFPNVQModel(**dict(dict(VQ_SMALL, lossconfig=DUMMY), **over)), "first_stage_model.").cuda().eval()


_SHARED = {}


def _model():
    if "m" not in _SHARED:
        _SHARED["m"] = _make()
    return _SHARED["m"]


def _img():
    return torch.from_numpy(golden("msvq_small")["img"]).cuda()


def _emb_loss_bound(g):
    """Relative bound on emb_loss: every scale's mean of squares moves by at most 2 * (ENC * max |h|) / rms(z_q - z) relative."""
    return max(2 * ENC * float(np.abs(g[f"h_{s}"]).max()) / float(g[f"rms_{s}"]) for s in range(len(E)))


@pytest.mark.gate
def test_encode_matches_reference_golden():
    g = golden("msvq_small")
    assert min(float(g[f"margin_{s}"].min()) for s in range(len(E))) > 1e-3      # the fixture's decisions are clear: equal codes are a fair demand
    m = _model()
    quant, emb_loss, info = m.encode(_img())
    assert info[0] == [None, None] and info[1] == [None, None] and len(info) == 3
    for s in range(len(E)):
        idx = info[2][s]
        assert idx.dtype == torch.int64 and idx.shape == g[f"idx_{s}"].shape and idx.is_cuda
        assert np.array_equal(idx.cpu().numpy(), g[f"idx_{s}"]), f"codes of scale {s}"
    assert quant.shape == g["quant"].shape and quant.dtype == torch.float32
    eq = _rel(quant, g["quant"])
    # channel order [fine .. coarse]: the first embed_dim[-1] channels are the FINE scale -- the fine codes' codebook rows at full
    # resolution; the rest is the coarse scale, constant over every 2 x 2 block (nearest upsampling)
    cb_fine = fill_module(_make_holder(), "first_stage_model.").ms_quantize[1].embedding.weight
    fine = cb_fine[torch.from_numpy(g["idx_1"])].reshape(2, 16, 16, E[1]).permute(0, 3, 1, 2)
    assert _rel(quant[:, :E[-1]], fine) < 1e-6
    coarse = quant[:, E[-1]:]
    assert torch.equal(coarse, coarse[:, :, ::2, ::2].repeat_interleave(2, 2).repeat_interleave(2, 3))
    assert not torch.equal(quant[:, :E[-1]], quant[:, :E[-1], ::2, ::2].repeat_interleave(2, 2).repeat_interleave(2, 3))
    assert emb_loss.dtype == torch.float32 and emb_loss.dim() == 0 and emb_loss.is_cuda
    el = abs(float(emb_loss) - float(g["emb_loss"])) / float(g["emb_loss"])
    print(f"msvq_small encode: quant rel err {eq:.2e} (bound {ENC:.0e}), emb_loss rel err {el:.2e} (bound {_emb_loss_bound(g):.2e}), codes equal")
    assert eq < ENC
    assert el < _emb_loss_bound(g)


def _make_holder():
    from frido_amd.models import MSFPNVQModel
    return MSFPNVQModel(**dict(VQ_SMALL, lossconfig=DUMMY))


@pytest.mark.gate
def test_forward_matches_reference_golden_and_replays_one_graph():
    g = golden("msvq_small")
    m = _model()
    x = _img()
    dec, diff, info = m(x)
    r = _rel(dec, g["dec"])
    print(f"msvq_small forward: dec rel err {r:.2e} (bound {PIX:.0e})")
    assert dec.shape == g["dec"].shape and r < PIX
    assert all(np.array_equal(info[2][s].cpu().numpy(), g[f"idx_{s}"]) for s in range(len(E)))
    quant, emb_loss, _ = m.encode(x)
    assert torch.equal(diff, emb_loss)                                   # the same kernels on the same maps: bit for bit
    rt = m.runtime()
    n = rt.graph_captures
    assert n >= 1
    dec2, diff2, info2 = m(x)                                            # replays the captured graph
    assert rt.graph_captures == n and torch.equal(dec2, dec) and torch.equal(diff2, diff) and torch.equal(info2[2][1], info[2][1])
    dec3, _, _ = m(x.flip(0))                                            # another batch, the same graph
    assert rt.graph_captures == n and _rel(dec3, g["dec"][::-1].copy()) < PIX
    assert torch.equal(m.decode(quant), dec)                             # decode(encode(x)[0]) == forward(x)[0]


def test_forward_with_aux_loss():
    g = golden("msvq_small")
    x = _img()
    dec_plain = _model()(x)[0]
    m = _make(use_aux_loss=True)
    dec, (aux, aux2), diff, info = m(x)
    ra, rb, r = _rel(aux, g["dec_aux"]), _rel(aux2, g["dec_aux2"]), _rel(dec, g["dec"])
    same = torch.equal(dec, dec_plain)
    print(f"msvq_small forward(use_aux_loss): dec {r:.2e}, dec_aux {ra:.2e}, dec_aux2 {rb:.2e} (bound {PIX:.0e}); dec bit-equal to the plain forward: {same}")
    assert ra < PIX and rb < PIX and r < PIX
    assert same, "rows of the batch-3B decode must not depend on their neighbours"
    assert abs(float(diff) - float(g["emb_loss"])) / float(g["emb_loss"]) < _emb_loss_bound(g)


def test_decode_agrees_with_the_interface_route_and_converts_to_uint8():
    from frido_amd.models import VQModelInterface
    m = _model()
    x = _img()
    dec = m(x)[0]
    v = fill_module(VQModelInterface(**VQ_SMALL, lossconfig=DUMMY), "first_stage_model.").cuda().eval()
    via = v.decode(v.encode(x))                                          # pre-quant [coarse .. fine] latent, quantised on the way in
    r = _rel(via, dec.cpu())
    print(f"msvq_small: VQModelInterface.decode(encode(x)) vs MSFPNVQModel.forward {r:.2e}")
    assert r < PIX
    quant = m.encode(x)[0]
    u8 = m.decode(quant, to_uint8=True)
    assert u8.dtype == torch.uint8 and u8.shape == (2, 64, 64, 3)
    want = ((dec.cpu() + 1) * 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    assert torch.equal(u8.cpu(), want)


@pytest.mark.parametrize("aux", [False, True], ids=["plain", "aux"])
def test_log_images(aux):
    g = golden("msvq_small")
    m = _make(use_aux_loss=True) if aux else _model()
    x = _img()
    batch = dict(image=x.permute(0, 2, 3, 1).contiguous(), file_name=["a", "b"])
    log = m.log_images(batch)
    assert sorted(log) == list(g["log_keys_aux" if aux else "log_keys"])
    assert sorted(m.log_images(dict(image=batch["image"]))) == [k for k in g["log_keys_aux" if aux else "log_keys"] if k != "file_name"]
    if not aux:
        assert [k for k in g["log_keys"] if k != "file_name"] == list(g["log_keys_nofile"])
    assert log["file_name"] == ["a", "b"] and torch.equal(log["inputs"], x) and _rel(log["reconstructions"], g["dec"]) < PIX
    assert len(log["codebook_info"]) == 1 and all(np.array_equal(log["codebook_info"][0][s].cpu().numpy(), g[f"idx_{s}"]) for s in range(len(E)))
    for k in ("reconstructions_0_3", "reconstructions_3_6"):
        r = _rel(log[k], g["log_" + k])
        print(f"msvq_small log_images[{k}] (aux={aux}): rel err {r:.2e} (bound {PIX:.0e})")
        assert log[k].shape == (2, 3, 64, 64) and r < PIX
    if aux:
        assert _rel(log["reconstructions_aux"][0], g["dec_aux"]) < PIX and _rel(log["reconstructions_aux"][1], g["dec_aux2"]) < PIX


def test_not_legacy_and_sane_index_shape():
    g, gn = golden("msvq_small"), golden("msvq_small_nl")
    m = _make(legacy=False, sane_index_shape=True, quant_beta=float(gn["quant_beta"]))
    quant, emb_loss, info = m.encode(_img())
    for s in range(len(E)):
        assert info[2][s].shape == gn[f"idx_{s}"].shape and info[2][s].dim() == 3
        assert np.array_equal(info[2][s].cpu().numpy(), gn[f"idx_{s}"])
    el = abs(float(emb_loss) - float(gn["emb_loss"])) / float(gn["emb_loss"])
    print(f"msvq_small_nl: emb_loss rel err {el:.2e} (bound {_emb_loss_bound(g):.2e})")
    assert el < _emb_loss_bound(g)
    assert _rel(quant, g["quant"]) < ENC
    _, _, info_f = m(_img())
    assert info_f[2][0].shape == gn["idx_0"].shape


def test_bf16_pair_build_runs():
    g = golden("msvq_small")
    m = _make(precision="bf16x3_bf16")
    assert m.planes == "bf16"
    dec, diff, info = m(_img())
    for s in range(len(E)):
        assert np.array_equal(info[2][s].cpu().numpy(), g[f"idx_{s}"]), f"codes of scale {s}"
    r = _rel(dec, g["dec"])
    print(f"msvq_small forward [bf16x3_bf16]: dec rel err {r:.2e} (bound {PIX_BF16P:.0e})")
    assert r < PIX_BF16P
    assert torch.equal(m.encode(_img())[1], diff)
