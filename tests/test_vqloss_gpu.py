"""frido_vq_commit_loss (frido_amd/csrc/vqloss.hip) through the C ABI on the MI355X: the codebook loss of MSFPNVQModel.encode against torch
float64 on the same inputs, its determinism, the independence of the scales and the capture / replay form.

Bound: the fp32 square of an fp32 difference carries at most 2 * 2^-24 + 2^-24 < 2^-22 relative error per element (both roundings), every
element is non-negative so the f64 sum keeps that, the f64 accumulation adds ~1e-13, the final rounding to fp32 2^-24: under 3e-7 in all;
asserted at 1e-6."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.gate]

from frido_amd import _lib  # noqa: E402
from frido_amd.vqloss import commit_loss_desc  # noqa: E402

REL = 1e-6
B = 2
# (npix, C, c0, e) per scale, coarse first
CASES = {
    "scalar_two_scales": [(B * 8 * 8, 6, 3, 3), (B * 16 * 16, 6, 3, 3)],       # e = 3 in rows of 6 at offset 3: scalar accesses, non-zero slice
    "vector_two_scales": [(B * 8 * 8, 8, 4, 4), (B * 16 * 16, 8, 4, 4)],       # multiples of 4: 16-byte accesses
    "one_pixel": [(1, 3, 0, 3)],                                               # fewer units than threads
    "ragged_257": [(257, 3, 0, 1)],                                            # 257 units: thread 0 owns two, the others one
    "ragged_257_vec": [(257, 4, 0, 4)],
    "many_workgroups": [(9001, 8, 4, 4), (4099, 5, 1, 3)],                     # 3 and 4 workgroups, ragged last strides
}


def _maps(case, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for npix, Cn, c0, e in CASES[case]:
        z = torch.randn(npix, Cn, generator=g, device="cuda") * 1.7
        zq = z + 0.4 * torch.randn(npix, Cn, generator=g, device="cuda")
        out.append((z, zq))
    return out


def _launch(case, maps, beta=0.25, legacy=True, scales=None, stream=None):
    """-> (means [n] f32, emb_loss 0-d f32) of one launch; scales: run only these of the case."""
    L = _lib.lib()
    sel = list(range(len(maps))) if scales is None else list(scales)
    ws = torch.full((_lib.VQLOSS_WS_BYTES // 8,), float("nan"), dtype=torch.float64, device="cuda")      # needs no initialisation
    means = torch.full((len(sel),), -1.0, device="cuda")
    total = torch.full((), -1.0, device="cuda")
    desc = commit_loss_desc([(maps[k][0].data_ptr(), maps[k][1].data_ptr()) + CASES[case][k] for k in sel], partials=ws.data_ptr(),
                            out=means.data_ptr(), emb_loss=total.data_ptr(), beta=beta, legacy=legacy)
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _lib.check(L.frido_vq_commit_loss(C.byref(desc), st), "frido_vq_commit_loss")
    return means, total, (desc, ws)


def _ref_means(case, maps):
    out = []
    for (z, zq), (npix, Cn, c0, e) in zip(maps, CASES[case]):
        out.append(float(((zq[:, c0:c0 + e].double() - z[:, c0:c0 + e].double()) ** 2).mean()))
    return out


def _expr(means, beta, legacy):
    """The reference's expression (quantize.py:287-291, msvqgan.py:153) in fp32 from given per-scale means."""
    b = np.float32(beta)
    total = np.float32(0.0)
    for m in means:
        m = np.float32(m)
        total = np.float32(total + (np.float32(m + np.float32(b * m)) if legacy else np.float32(np.float32(b * m) + m)))
    return total


@pytest.mark.parametrize("legacy", [True, False], ids=["legacy", "not_legacy"])
@pytest.mark.parametrize("case", list(CASES))
def test_means_match_float64_and_the_total_is_the_reference_expression(case, legacy):
    maps = _maps(case)
    beta = 0.25 if legacy else 0.4
    means, total, _ = _launch(case, maps, beta=beta, legacy=legacy)
    torch.cuda.synchronize()
    got, ref = means.cpu().numpy(), _ref_means(case, maps)
    for k, (a, r) in enumerate(zip(got, ref)):
        err = abs(float(a) - r) / r
        print(f"vq_commit_loss {case} scale {k} legacy={legacy}: mean {float(a):.9g}, float64 {r:.9g}, rel err {err:.2e}")
        assert err <= REL, (case, k)
    want = _expr(got, beta, legacy)
    assert total.dtype == torch.float32 and total.dim() == 0
    assert np.float32(total.item()).tobytes() == want.tobytes(), (float(total), float(want))


@pytest.mark.parametrize("case", ["scalar_two_scales", "vector_two_scales", "many_workgroups"])
def test_two_launches_give_the_same_bits(case):
    maps = _maps(case)
    a = _launch(case, maps)
    b = _launch(case, maps)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("case", ["scalar_two_scales", "vector_two_scales", "many_workgroups"])
def test_a_scale_does_not_depend_on_its_neighbours(case):
    maps = _maps(case)
    both = _launch(case, maps)
    alone0 = _launch(case, maps, scales=[0])
    alone1 = _launch(case, maps, scales=[1])
    swapped = _launch(case, maps, scales=[1, 0])
    torch.cuda.synchronize()
    assert torch.equal(both[0][:1], alone0[0]) and torch.equal(both[0][1:], alone1[0])
    assert torch.equal(swapped[0], both[0].flip(0))


@pytest.mark.parametrize("case", ["scalar_two_scales", "vector_two_scales"])
def test_captured_replay_equals_the_eager_bits(case):
    L = _lib.lib()
    _lib.check(L.frido_init(), "frido_init")
    maps = _maps(case)
    eager_means, eager_total, _ = _launch(case, maps)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sp = side.cuda_stream
        ws = torch.zeros(_lib.VQLOSS_WS_BYTES // 8, dtype=torch.float64, device="cuda")
        means, total = torch.full((2,), -1.0, device="cuda"), torch.full((), -1.0, device="cuda")
        desc = commit_loss_desc([(z.data_ptr(), zq.data_ptr()) + CASES[case][k] for k, (z, zq) in enumerate(maps)], partials=ws.data_ptr(),
                                out=means.data_ptr(), emb_loss=total.data_ptr(), beta=0.25, legacy=True)
        _lib.check(L.frido_capture_begin(sp), "frido_capture_begin")
        rc = L.frido_vq_commit_loss(C.byref(desc), sp)
        h = C.c_void_p()
        rc_end = L.frido_capture_end(sp, C.byref(h))
        assert rc == 0 and rc_end == 0, L.frido_last_error()
        try:
            side.synchronize()
            assert float(total) == -1.0                      # captured, not run
            for _ in range(2):
                _lib.check(L.frido_graph_launch(h, sp), "frido_graph_launch")
                side.synchronize()
                assert torch.equal(means, eager_means) and torch.equal(total, eager_total)
                means.fill_(-1.0)
        finally:
            L.frido_graph_destroy(h)
    torch.cuda.current_stream().wait_stream(side)
