"""CPU-side checks of LPIPS: the float64 restatement (tests/lpips_ref.py) against the fixture captured from the reference's own module
(tests/golden/lpips_ref.npz), the holder's state_dict, the local-file loaders, the refusals, and the four launchers of
include/frido_lpips.h as far as they go without a device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import lpips_ref as R
from frido_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "lpips_ref.npz"))


@functools.lru_cache(maxsize=None)
def _sd():
    from frido_amd.models import LPIPS
    return R.filled_state_dict(LPIPS())


# ---- the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(R.CASES)), ids=[str(c) for c in R.CASES])
def test_restatement_matches_the_reference_golden(ci):
    """The reference ran in float32; the restatement in float64 may differ from it by what float32 costs.  That cost is measured on the
    restatement itself (float32 run against float64 run, same weights and images); the bound is 4 x it: the reference's float32 run
    and the restatement's float32 run order their sums differently (torch's conv2d picks its algorithm per shape and dtype)."""
    case = R.CASES[ci]
    assert tuple(GOLD["cases"][ci]) == case
    x, y = R.images(*case, R.case_seed(case))
    tot64, per64, fx64, fy64 = R.lpips_ref(_sd(), x, y)
    tot32, per32, fx32, fy32 = R.lpips_ref(_sd(), x, y, dtype=torch.float32)
    e_per = float(((per32.double() - per64) / per64).abs().max())
    e_tot = float(((tot32.double() - tot64) / tot64).abs().max())
    d_per = float(((torch.from_numpy(GOLD[f"per_layer_{ci}"]).double() - per64) / per64).abs().max())
    d_tot = float(((torch.from_numpy(GOLD[f"out_{ci}"]).double() - tot64) / tot64).abs().max())
    print(f"lpips restatement {case}: golden vs f64 per layer {d_per:.3e} (f32 restatement {e_per:.3e}), total {d_tot:.3e} ({e_tot:.3e})")
    e = max(e_per, e_tot)           # the total's own float32 error is often far below a layer's: one bound from the larger
    assert e > 0 and d_per <= 4 * e and d_tot <= 4 * e
    for k in range(5):
        for tag, f64, f32 in (("x", fx64[k], fx32[k]), ("y", fy64[k], fy32[k])):
            idx = R.sample_index(f64.numel(), k, case)
            scale = float(f64.abs().max())
            ef = float((f32.double() - f64).abs().max()) / scale
            df = float((torch.from_numpy(GOLD[f"feat_{tag}_{ci}_{k}"]).double() - f64.flatten()[idx]).abs().max()) / scale
            assert ef > 0 and df <= 4 * ef, (k, tag, df, ef)


def test_every_layer_contributes_and_the_normalisation_is_well_conditioned():
    """What the GPU bounds rest on: no layer's value is negligible beside the total, and no pixel's feature norm is small beside its
    layer's mean norm (a small norm would amplify the features' rounding error through the division)."""
    for case in R.CASES:
        x, y = R.images(*case, R.case_seed(case))
        tot, per, fx, fy = R.lpips_ref(_sd(), x, y)
        assert float(per.min()) > 0.02 * float(tot.max()), (case, per)
        for k in range(5):
            for f in (fx[k], fy[k]):
                n = torch.sqrt((f ** 2).sum(1))
                assert float(n.min()) >= 0.3 * float(n.mean()), (case, k, float(n.min() / n.mean()))


def test_wrong_variants_of_the_layer_formula_are_far_away():
    """layer_ref's keywords are the near misses the GPU test uses: each moves the result, in float64, by far more than float32 does."""
    g = torch.Generator().manual_seed(5)
    f0 = torch.rand(2, 64, 3, 3, generator=g, dtype=torch.float64)
    f1 = torch.rand(2, 64, 3, 3, generator=g, dtype=torch.float64)
    f0[0, :, 0, 0] *= 1e-6                             # a pixel of tiny features (norm ~ 5e-6): where eps inside / outside the root differ
    f0[1, :, 0, 0] *= 1e-6                             # (sqrt(s + 1e-10) ~ 1e-5 against sqrt(s) + 1e-10 ~ 5e-6; on O(1) features they agree to 1e-10)
    w = torch.rand(64, generator=g, dtype=torch.float64)
    ref = R.layer_ref(f0, f1, w)
    for kw in (dict(eps_inside=True), dict(normalise=False), dict(diff_first=True), dict(unit_weights=True), dict(pad_count=7)):
        assert float(((R.layer_ref(f0, f1, w, **kw) - ref) / ref).abs().max()) > 1e-5, kw


# ---- the holder ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_dropout", [True, False])
def test_state_dict_is_the_references(use_dropout):
    from frido_amd.models import LPIPS
    m = LPIPS(use_dropout=use_dropout)
    keys = [str(k) for k in GOLD[f"keys_dropout_{int(use_dropout)}"]]
    shapes = [tuple(int(s) for s in str(v).split(",")) for v in GOLD[f"shapes_dropout_{int(use_dropout)}"]]
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(zip(keys, shapes))
    assert f"lin3.model.{1 if use_dropout else 0}.weight" in keys and "scaling_layer.shift" in keys
    assert not m.training and all(not p.requires_grad for p in m.parameters())
    assert torch.equal(m.scaling_layer.shift.flatten(), torch.Tensor([-.030, -.088, -.188]))
    assert torch.equal(m.scaling_layer.scale.flatten(), torch.Tensor([.458, .448, .450]))
    # the `loss.perceptual_loss.*` keys of a taming checkpoint, prefix stripped, load strictly
    assert not m.load_state_dict({k: torch.zeros(s) for k, s in zip(keys, shapes)}, strict=True).missing_keys


def test_local_checkpoints_map_onto_the_slices(tmp_path):
    from frido_amd.lpips import VGG_SLICES
    from frido_amd.models import LPIPS
    g = torch.Generator().manual_seed(9)
    lin = {f"lin{k}.model.1.weight": torch.rand(1, c, 1, 1, generator=g) for k, c in enumerate(R.CHNS)}
    vgg, cin = {}, 3
    for convs in VGG_SLICES:
        for idx, cout in convs:
            vgg[f"features.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g)
            vgg[f"features.{idx}.bias"] = torch.randn(cout, generator=g)
            cin = cout
    vgg["classifier.0.weight"] = torch.zeros(4, 4)              # passed over
    torch.save(lin, tmp_path / "vgg.pth")
    torch.save(vgg, tmp_path / "vgg16.pth")
    for use_dropout in (True, False):                           # a vgg.pth written under use_dropout=True loads into either form
        m = LPIPS(use_dropout=use_dropout, lin_ckpt=str(tmp_path / "vgg.pth"), vgg_ckpt=str(tmp_path / "vgg16.pth"))
        sd = m.state_dict()
        for k in range(5):
            assert torch.equal(sd[R.lin_key(sd, k)], lin[f"lin{k}.model.1.weight"])
        for si, convs in enumerate(VGG_SLICES):
            for idx, _ in convs:
                for leaf in ("weight", "bias"):
                    assert torch.equal(sd[f"net.slice{si + 1}.{idx}.{leaf}"], vgg[f"features.{idx}.{leaf}"])
        assert all(not p.requires_grad for p in m.parameters())
    m = LPIPS.from_pretrained(path=str(tmp_path / "vgg.pth"))
    assert torch.equal(m.state_dict()["lin2.model.1.weight"], lin["lin2.model.1.weight"])
    del vgg["features.12.bias"]
    torch.save(vgg, tmp_path / "broken.pth")
    with pytest.raises(KeyError, match=r"features\.12\.bias"):
        LPIPS(vgg_ckpt=str(tmp_path / "broken.pth"))


# ---- refusals, by their words --------------------------------------------------------------------------
def test_refusals_name_themselves():
    from frido_amd.models import LPIPS
    from frido_amd.pipeline import reconstruction_metrics
    m = LPIPS()
    with pytest.raises(NotImplementedError, match="downloads vgg.pth"):
        LPIPS.from_pretrained()
    with pytest.raises(NotImplementedError, match="only 'vgg_lpips'"):
        LPIPS.from_pretrained("alex")
    with pytest.raises(NotImplementedError, match="downloads vgg.pth"):
        m.load_from_pretrained()
    with pytest.raises(NotImplementedError, match="use_dropout=True.*Dropout"):
        m.train()
    assert m.eval() is m and not m.training
    assert LPIPS(use_dropout=False).train().training            # nothing to drop: allowed
    ok = torch.zeros(2, 3, 16, 16)
    for bad in (torch.zeros(2, 3, 16), torch.zeros(2, 4, 16, 16), torch.zeros(3, 16, 16), "image"):
        with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
            m(bad, ok)
        with pytest.raises(ValueError, match=r"target must be a \[B, 3, H, W\]"):
            m.per_layer(ok, bad)
    with pytest.raises(ValueError, match="differ in shape"):
        m(ok, torch.zeros(2, 3, 16, 20))
    with pytest.raises(ValueError, match="differ in shape"):
        m(ok, torch.zeros(1, 3, 16, 16))
    for small in ((15, 16), (16, 8)):
        with pytest.raises(ValueError, match="at least 16"):
            m(torch.zeros(1, 3, *small), torch.zeros(1, 3, *small))
    with pytest.raises(_lib.FridoHipError, match="no CPU fallback"):
        m(ok, ok)
    with pytest.raises(_lib.FridoHipError, match="no CPU fallback"):
        m.per_layer(ok, ok)
    with pytest.raises(ValueError, match="must be a frido_amd.models.LPIPS"):
        reconstruction_metrics(m, ok, torch.nn.Identity())
    with pytest.raises(ValueError, match="MSFPNVQModel or a VQModelInterface"):
        reconstruction_metrics(torch.nn.Identity(), ok, m)


def test_validation_step_still_refuses_as_it_did():
    import inspect
    from frido_amd.models import MSFPNVQModel
    assert "LPIPS + a PatchGAN discriminator" in inspect.getsource(MSFPNVQModel.validation_step)


def test_alias_imports():
    import taming.modules.losses as losses
    from frido_amd.models import LPIPS, DummyLoss
    from taming.modules.losses.lpips import LPIPS as alias
    assert alias is LPIPS and losses.LPIPS is LPIPS and losses.DummyLoss is DummyLoss


# ---- the launchers, without a device -------------------------------------------------------------------
def test_descriptor_sizes_on_both_libraries():
    from frido_amd import lpips
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        for name, (struct, sizeof) in lpips.LAUNCHERS.items():
            assert getattr(L, sizeof)() == C.sizeof(struct), (planes, name)
        assert set(lpips._fns(planes)) == set(lpips.LAUNCHERS)
    assert C.sizeof(lpips.FridoLpipsScale) == 3 * 8 + 3 * 4 + 6 * 4 + 4      # three pointers, B H W, shift / scale, tail padding


def test_bad_descriptors_are_turned_away_before_a_device_is_touched():
    from frido_amd import lpips
    buf = (C.c_double * 64)()
    base = (C.addressof(buf) + 15) & ~15
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        fns = lpips._fns(planes)

        def refused(name, desc, words):
            assert fns[name](C.byref(desc), None) == -1 and words in L.frido_last_error(), (name, L.frido_last_error())      # FRIDO_EINVAL

        for name, (struct, _) in lpips.LAUNCHERS.items():                  # a zeroed descriptor: null pointers
            refused(name, struct(), name.encode() + b": bad arguments")
        for kw, words in ((dict(x=None), b"bad arguments"), (dict(y=None), b"bad arguments"), (dict(dst=None), b"bad arguments"),
                          (dict(B=0), b"bad arguments"), (dict(H=0), b"bad arguments")):
            d = lpips.scale_desc(base, base, base, 1, 4, 4)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_lpips_scale", d, words)
        d = lpips.scale_desc(base, base, base, 1, 4, 4, scale=(0.5, 0.0, 0.5))
        refused("frido_lpips_scale", d, b"a zero scale")
        for kw, words in ((dict(C=6), b"multiple of 4"), (dict(H=1), b"2 x 2 window"), (dict(W=1), b"2 x 2 window"), (dict(src=None), b"bad arguments"),
                          (dict(dst=base + 4), b"16-byte aligned"), (dict(B=0), b"bad arguments")):
            d = lpips.maxpool_desc(base, base, 1, 4, 4, 8)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_maxpool2", d, words)
        for kw, words in ((dict(C=66), b"multiple of 4"), (dict(nblk=0), b"workgroups per sample"), (dict(nblk=5), b"workgroups per sample"),
                          (dict(w=None), b"bad arguments"), (dict(partials=None), b"bad arguments"), (dict(f1=base + 8), b"16-byte aligned"),
                          (dict(B=70000), b"65535"), (dict(HW=0), b"bad arguments")):
            d = lpips.layer_desc(base, base, base, base, 1, 4, 64, 2)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_lpips_layer", d, words)
        d = lpips.finish_desc(base, base, base, 1, [1, 1, 0, 1, 1], [4, 4, 4, 4, 4])
        refused("frido_lpips_finish", d, b"every layer")
        d = lpips.finish_desc(base, base, None, 1, [1] * 5, [4] * 5)
        refused("frido_lpips_finish", d, b"bad arguments")
    d = lpips.scale_desc(16, 32, 48, 2, 8, 8)
    assert list(d.shift) == torch.tensor(R.SHIFT, dtype=torch.float32).tolist()      # the module's float32 buffers, bit for bit
    assert list(d.scale) == torch.tensor(R.SCALE, dtype=torch.float32).tolist()
    assert [lpips.layer_blocks(hw) for hw in (1, 32, 33, 1024, 65536)] == [1, 1, 2, 32, 256]
    assert lpips.plane_sizes(40, 36) == [(40, 36), (20, 18), (10, 9), (5, 4), (2, 2)]


def test_the_op_table_header_does_not_know_the_launches():
    """frido_hip.h is the op-kind ABI (tests/test_opkinds_host.py pins it): LPIPS's launches live in a header of their own."""
    hip = open(os.path.join(REPO, "include", "frido_hip.h")).read()
    for name in ("lpips", "maxpool", "FridoLpips", "FridoMaxPool2"):
        assert name not in hip
    assert _lib.ABI_VERSION == 8 and _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36
    assert not [s for s in _lib.EXPORTS if "lpips" in s or "maxpool" in s]
    assert not [s for s in _lib.STRUCTS if "Lpips" in s or "MaxPool" in s]
    hdr = open(os.path.join(REPO, "include", "frido_lpips.h")).read()
    assert '#include "frido_hip.h"' in hdr
    assert _lib._parse_structs(_lib._strip_comments(hdr)).keys() == {"FridoLpipsScale", "FridoMaxPool2", "FridoLpipsLayer", "FridoLpipsFinish"}
    mk = open(os.path.join(REPO, "frido_amd", "csrc", "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0].split()
    assert srcs[-1] == "lpips.hip" and srcs[-2] == "vision.hip"      # appended: the status words are numbered in link order
    assert "lpips.o obj_bf16p/lpips.o: ../../include/frido_lpips.h" in mk
    src = open(os.path.join(REPO, "frido_amd", "csrc", "lpips.hip")).read()
    assert '#include "launch.h"' in src and "common.h" not in src and "atomic" not in src.lower().replace("no atomics", "")
