"""The host reference of the noise generator (tests/philox_ref.py) against published known answers, and its edge words.  No GPU: the GPU
tests (test_philox_gpu.py) then compare frido_randn and the sampler kernels' in-kernel draws with this reference."""
import numpy as np

import philox_ref as P

# Random123's known-answer vectors for philox4x32-10 (its kat_vectors file): counter, key, result
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox4x32_10_known_answers():
    for ctr, key, want in KAT:
        got = P.philox4x32(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert tuple(int(v) for v in got) == want, (ctr, key, [hex(int(v)) for v in got])
    # vectorised over a leading shape: the same three answers from one call
    got = P.philox4x32(np.array([c for c, _, _ in KAT], dtype=np.uint64), np.array([k for _, k, _ in KAT], dtype=np.uint64))
    assert got.shape == (3, 4) and [tuple(int(v) for v in row) for row in got] == [w for _, _, w in KAT]
    # nine rounds is another function (the wrong variant the GPU tests hold up against their bound)
    assert tuple(int(v) for v in P.philox4x32(np.zeros(4, np.uint64), np.zeros(2, np.uint64), rounds=9)) != KAT[0][2]


def test_counter_layout():
    """{grp, draw, sample lo, sample hi ^ (stream << 20)} / {seed lo, seed hi}, negative samples as their two's-complement bits."""
    ctr, key = P.counter(seed=2 ** 64 - 1, sample=2 ** 32 + 1, draw=6, stream=65, grp=9)
    assert [int(v) for v in ctr] == [9, 6, 1, 1 ^ (65 << 20)] and [int(v) for v in key] == [0xffffffff, 0xffffffff]
    ctr, key = P.counter(seed=2 ** 32 + 5, sample=-1, draw=0, stream=1, grp=np.array([0, 3]))
    assert ctr.shape == (2, 4) and [int(v) for v in ctr[1]] == [3, 0, 0xffffffff, 0xffffffff ^ (1 << 20)]
    assert [int(v) for v in key] == [5, 1]
    ctr, _ = P.counter(seed=0, sample=0, draw=6, stream=0, grp=9, swap_grp_draw=True)
    assert [int(v) for v in ctr] == [6, 9, 0, 0]


def test_box_muller_edge_words():
    """c = 0 and c = 2^32 - 1 in every position: finite, |v| <= sqrt(64 ln 2).  A radius word of 0 gives the largest radius (u = 2^-32), one
    of 2^32 - 1 gives u = 1 exactly (float(c) rounds to 2^32, + 1 is absorbed) and radius 0; an angle word of 2^32 - 1 gives the angle
    6.2831855f, just past 2 pi."""
    lo, hi = 0, 0xffffffff
    words = np.array([[a, b, c, d] for a in (lo, hi) for b in (lo, hi) for c in (lo, hi) for d in (lo, hi)], dtype=np.uint64)
    v = P.box_muller(words)
    assert np.isfinite(v).all() and float(np.abs(v).max()) <= P.VMAX
    assert abs(P.VMAX - 6.6604) < 1e-4
    r0 = P.box_muller(np.array([lo, lo, hi, lo], dtype=np.uint64))
    assert r0[0] == P.VMAX and r0[1] == 0.0 and r0[2] == 0.0 and r0[3] == 0.0          # angle 0: cos 1, sin 0; radius word hi: radius 0
    past = P.box_muller(np.array([lo, hi, lo, hi], dtype=np.uint64))
    assert 0.0 < past[1] < 2e-6 and past[0] < P.VMAX                                   # sin(6.2831855f) = +1.7e-7 * radius
    # inner words next to the edges stay inside the bound too
    near = np.array([[1, 1, 2, 2], [hi - 1, hi - 1, hi - 255, hi - 255], [128, hi - 128, 129, 127]], dtype=np.uint64)
    assert float(np.abs(P.box_muller(near)).max()) <= P.VMAX


def test_reference_is_gaussian_and_numbering_is_consistent():
    """The statement itself: moments of 2^16 draws, and the two numberings (flat fill, per-pixel groups) reduce to randn4."""
    v = P.randn_fill(1234, 0, 0, 4096, np.arange(1 << 14))
    assert abs(v.mean()) < 0.02 and abs(v.std() - 1.0) < 0.02 and abs((v ** 4).mean() - 3.0) < 0.15
    # flat group 1024 + 7 with per_sample 4096 is group 7 of sample sample0 + 1
    assert np.array_equal(P.randn_fill(9, 3, 1, 4096, [1024 + 7])[0], P.randn4(9, 4, 0, 1, 7))
    nz = P.sampler_noise(9, 3, 1, 6, B=2, HW=5, nch=6)
    assert nz.shape == (2, 5, 6)
    assert np.array_equal(nz[1, 4, 4:6], P.randn4(9, 4, 6, 1, 4 * 2 + 1)[:2])          # channels 4, 5: group p * 2 + 1, elements 0, 1
    assert np.array_equal(nz[0, 2, :4], P.randn4(9, 3, 6, 1, 2 * 2 + 0))
    # the wrong variants differ by O(1)
    assert np.abs(P.randn_fill(9, 3, 1, 4096, np.arange(64), rounds=9) - P.randn_fill(9, 3, 1, 4096, np.arange(64))).max() > 1.0
    assert np.abs(P.sampler_noise(9, 3, 1, 6, 2, 5, 6, swap_grp_draw=True) - nz).max() > 1.0
